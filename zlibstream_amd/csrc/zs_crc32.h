// zs_crc32.h -- CRC-32 (IEEE 802.3, reflected polynomial 0xEDB88320; zlib's crc32), the parts that the device kernels
// (zs_crc32.hip) and the host (the engine's table set-up, the PNG chunk walk, tests/cpp/test_crc32.cpp) share: the byte
// step, the table generator, x^n mod P, the GF(2) multiply and the combine; and the PNG chunk walk itself (host only).
//
// Representation.  A register value holds a polynomial over GF(2) of degree < 32, bit 31 the coefficient of x^0 (reflected).
// Feeding a byte b to the register c is  c' = T0[(c ^ b) & 255] ^ (c >> 8);  feeding n zero bytes multiplies c by x^(8n)
// mod P.  raw(m), the register after message m from a zero register, is linear in m, leading zero bytes leave it zero, and
//     register(c0, a ++ b) = raw(a) * x^(8 |b|)  ^  raw(b)  ^  c0 * x^(8 (|a| + |b|))
// which is all the kernels use: a span is cut into tiles, every tile's raw value is scaled by x^(8 * bytes behind it) and
// the span's register is the XOR of them.  zlib's crc32(seed, buf, len) is ~register(~seed, buf).
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "zs_core.h"

namespace zs {

constexpr uint32_t kCrc32Poly = 0xEDB88320u;
constexpr uint32_t kCrc32One = 0x80000000u;  // x^0

// eight steps of the register: entry i of the byte table T0 is crc32_byte_step(i)
ZS_HD uint32_t crc32_byte_step(uint32_t c) {
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (kCrc32Poly & (0u - (c & 1u)));
    return c;
}
// table-free form of the byte step for cold paths
ZS_HD uint32_t crc32_feed_byte(uint32_t c, uint32_t b) { return crc32_byte_step((c ^ b) & 0xFF) ^ (c >> 8); }
// entry i of slice table t: the register after byte i and t zero bytes, from zero (t = 0: T0)
ZS_HD uint32_t crc32_table_entry(int t, uint32_t i) {
    uint32_t c = crc32_byte_step(i);
    for (int k = 0; k < t; k++) c = crc32_byte_step(c & 0xFF) ^ (c >> 8);
    return c;
}

// a * b mod P
ZS_HD uint32_t crc32_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 31; i >= 0; i--) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (kCrc32Poly & (0u - (b & 1u)));
    }
    return p;
}

// x2n[k] = x^(2^k) mod P, k = 0..31 (x^(2^32) = x: the table is used cyclically)
ZS_HD void crc32_x2n_table(uint32_t *x2n) {
    uint32_t p = kCrc32One >> 1;  // x^1
    for (int k = 0; k < 32; k++) {
        x2n[k] = p;
        p = crc32_mul(p, p);
    }
}
// x^(n * 2^k) mod P
template <class Tab>
ZS_HD uint32_t crc32_xpow(const Tab &x2n, uint64_t n, unsigned k) {
    uint32_t p = kCrc32One;
    for (; n; n >>= 1, k++)
        if (n & 1) p = crc32_mul(x2n[k & 31], p);
    return p;
}
// zlib's crc32_combine: the CRC of a ++ b from crc(a), crc(b) and |b|
template <class Tab>
ZS_HD uint32_t crc32_combine(const Tab &x2n, uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return crc32_mul(crc32_xpow(x2n, len_b, 3), crc_a) ^ crc_b;
}

// zlib's crc32(seed, buf, len) a byte at a time; t0: the 256 entries of T0
template <class Tab>
ZS_HD uint32_t crc32_bytes(const Tab &t0, uint32_t seed, const uint8_t *p, uint64_t len) {
    uint32_t c = ~seed;
    for (uint64_t i = 0; i < len; i++) c = t0[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}
// ... and without a table (cold paths: a chunk type, IHDR, IEND)
ZS_HD uint32_t crc32_bytes_slow(uint32_t seed, const uint8_t *p, uint64_t len) {
    uint32_t c = ~seed;
    for (uint64_t i = 0; i < len; i++) c = crc32_feed_byte(c, p[i]);
    return ~c;
}

// ---- the tile kernel's geometry (zs_crc32.hip) ----
constexpr int kCrcTile = 8192;      // bytes of a span one wave takes at a time
constexpr int kCrcWaves = 4;        // waves of a workgroup = tiles it takes in one pass
constexpr int kCrcStride = 64 * 16; // strided form: bytes between two words of a lane
constexpr int kCrcPow128 = kCrcTile / 16 + 2;  // entries of the table x^(128 q): a tile and its head word
// The tables the kernels read, in one device allocation (uint32 each):
//   slice[16][256]   crc32_table_entry(t, i)
//   shift[4][256]    byte j of a register moved kCrcStride bytes on: T0[i] * x^(8 (kCrcStride - 1 - j))
//   pow128[kCrcPow128]  x^(128 q)      pow8[16]  x^(8 r)      x2n[32]
constexpr int kCrcTabSlice = 0, kCrcTabShift = 16 * 256, kCrcTabPow128 = 20 * 256, kCrcTabPow8 = kCrcTabPow128 + kCrcPow128,
              kCrcTabX2n = kCrcTabPow8 + 16, kCrcTabWords = kCrcTabX2n + 32;
inline void crc32_fill_tables(uint32_t *t) {
    uint32_t x2n[32];
    crc32_x2n_table(x2n);
    for (uint32_t i = 0; i < 256; i++) t[kCrcTabSlice + i] = crc32_byte_step(i);
    for (int s = 1; s < 16; s++)
        for (uint32_t i = 0; i < 256; i++) {
            const uint32_t c = t[kCrcTabSlice + (s - 1) * 256 + i];
            t[kCrcTabSlice + s * 256 + i] = t[kCrcTabSlice + (c & 0xFF)] ^ (c >> 8);
        }
    for (int j = 0; j < 4; j++) {
        const uint32_t f = crc32_xpow(x2n, (uint64_t)(kCrcStride - 1 - j), 3);
        for (uint32_t i = 0; i < 256; i++) t[kCrcTabShift + j * 256 + i] = crc32_mul(t[kCrcTabSlice + i], f);
    }
    for (int q = 0; q < kCrcPow128; q++) t[kCrcTabPow128 + q] = crc32_xpow(x2n, (uint64_t)q, 7);
    for (int r = 0; r < 16; r++) t[kCrcTabPow8 + r] = crc32_xpow(x2n, (uint64_t)r, 3);
    for (int k = 0; k < 32; k++) t[kCrcTabX2n + k] = x2n[k];
}

// One span of a batch.  src: `len` bytes on the device, any alignment; init: the register the span starts from (~seed).
// dst (may be null): the span's bytes from byte `skip` on are also copied there, any alignment.  frame (may be null): a
// PNG chunk is closed around the copy -- big-endian length and `type` at frame, the data at frame + 8 = dst, the
// big-endian CRC behind it (the finishing launch writes the twelve bytes).  has_prefix: four more bytes, `prefix` big-endian
// (an fdAT's sequence number), stand between the type and the data -- the length field counts them, the data lies at
// frame + 12 = dst, and the CRC covers them: the host seeds init with the type and the prefix, as it seeds it with the type
// alone for a chunk without one.
struct Crc32Span {
    const uint8_t *src;
    uint8_t *dst, *frame;
    int64_t len;
    uint32_t init, skip, type, prefix;
    uint32_t has_prefix, pad;
};
ZS_HD int64_t crc32_span_tiles(int64_t len) { return (len + kCrcTile - 1) / kCrcTile; }

// the span of flat tile t: the last i with tile_off[i] <= t (spans without tiles share their successor's offset)
template <class Off>
ZS_HD int crc32_tile_span(const Off &tile_off, int n, uint32_t t) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_off[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- PNG files (PNG specification 5: signature, chunk layout; 11.2.2: IHDR) ----
ZS_HD int png_channels(int color_type) { return color_type == 0 || color_type == 3 ? 1 : color_type == 2 ? 3 : color_type == 4 ? 2 : color_type == 6 ? 4 : 0; }
// the (color type, bit depth) pairs of table 11.1
ZS_HD bool png_color_ok(int color_type, int bit_depth) {
    const bool d8_16 = bit_depth == 8 || bit_depth == 16, d1_8 = bit_depth == 1 || bit_depth == 2 || bit_depth == 4 || bit_depth == 8;
    switch (color_type) {
    case 0: return d1_8 || bit_depth == 16;
    case 3: return d1_8;
    case 2: case 4: case 6: return d8_16;
    default: return false;
    }
}
ZS_HD uint32_t png_be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
ZS_HD void png_put_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }
constexpr uint32_t png_type(char a, char b, char c, char d) { return (uint32_t)(uint8_t)a | (uint32_t)(uint8_t)b << 8 | (uint32_t)(uint8_t)c << 16 | (uint32_t)(uint8_t)d << 24; }
constexpr uint32_t kPngIHDR = png_type('I', 'H', 'D', 'R'), kPngPLTE = png_type('P', 'L', 'T', 'E'), kPngIDAT = png_type('I', 'D', 'A', 'T'),
                   kPngIEND = png_type('I', 'E', 'N', 'D');
constexpr int64_t kPngMaxChunk = 0x7FFFFFFF;  // a chunk's data length (PNG specification 5.3)

// Closes a chunk around `n` data bytes that are in place: the big-endian length and the type at f, the prefix (if any) behind
// them, the big-endian CRC behind the data -- twelve bytes, or sixteen.  What the finishing launch of KC does per framed span
// (zs_crc32.hip), and tests/cpp/test_png_diff.cpp on the host.
ZS_HD void png_close_chunk(uint8_t *f, uint32_t n, uint32_t type, bool has_prefix, uint32_t prefix, uint32_t crc) {
    png_put_be32(f, has_prefix ? n + 4 : n);
    f[4] = (uint8_t)type, f[5] = (uint8_t)(type >> 8), f[6] = (uint8_t)(type >> 16), f[7] = (uint8_t)(type >> 24);
    if (has_prefix) png_put_be32(f + 8, prefix);
    png_put_be32(f + (has_prefix ? 12 : 8) + n, crc);
}

// bytes of the file that holds a zlib stream of idat_len bytes in IDAT chunks of at most idat_chunk_bytes data bytes
// (0: one chunk; an empty stream still gets one chunk) and extra_len bytes of caller chunks; -1 for bad arguments
inline int64_t png_file_bound(int64_t idat_len, int64_t idat_chunk_bytes, int64_t extra_len) {
    if (idat_len < 0 || extra_len < 0 || idat_chunk_bytes < 0 || idat_chunk_bytes > kPngMaxChunk) return -1;
    if (idat_chunk_bytes == 0 && idat_len > kPngMaxChunk) return -1;
    if (idat_len > (int64_t)1 << 60 || extra_len > (int64_t)1 << 60) return -1;
    const int64_t chunks = idat_chunk_bytes == 0 || idat_len == 0 ? 1 : (idat_len + idat_chunk_bytes - 1) / idat_chunk_bytes;
    return 8 + 25 + extra_len + idat_len + 12 * chunks + 12;
}
// a sequence of complete chunks by its length fields alone
inline bool png_chunks_well_formed(const uint8_t *p, int64_t len) {
    int64_t at = 0;
    while (at < len) {
        if (len - at < 12) return false;
        const int64_t n = png_be32(p + at);
        if (n > kPngMaxChunk || n > len - at - 12) return false;
        at += 12 + n;
    }
    return true;
}

// What the chunk walk finds in one file.  Mirrors zs_png_info of the C ABI field for field (zs_engine.hip asserts it).
struct PngFileInfo {
    int64_t width, height;
    int bit_depth, color_type, interlace, bits_per_pixel;
    int64_t idat_bytes, pixel_bytes;
    int64_t n_idat;
};
// one chunk the device is to check (critical chunks) or gather (IDAT): offsets into the file
struct PngChunkRef {
    uint32_t type;
    int64_t at;    // of the chunk's length field
    int64_t len;   // of its data
};
// Walks the chunk chain of a file in host memory: signature, IHDR first and valid, the IDAT run, IEND.  Ancillary chunks
// are stepped over by their length fields (never interpreted, their CRCs never read).  Returns true and fills `info`, or
// false with the reason in msg.  emit(ref) is called for every critical chunk (IHDR, PLTE, IDAT, IEND) in file order;
// check_crc: critical chunks' CRCs are verified here on the host (zs_png_file_info) rather than left to the device.
template <class Emit>
inline bool png_walk_file(const uint8_t *f, int64_t len, PngFileInfo *info, char *msg, size_t msg_cap, bool check_crc, Emit emit) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    memset(info, 0, sizeof *info);
    if (len < 8 || memcmp(f, sig, 8) != 0) return snprintf(msg, msg_cap, "bad signature"), false;
    int64_t at = 8;
    bool first = true, in_idat = false, idat_done = false, ended = false;
    while (at < len) {
        if (len - at < 8) return snprintf(msg, msg_cap, "truncated chunk at offset %lld", (long long)at), false;
        const int64_t n = png_be32(f + at);
        uint32_t type;
        memcpy(&type, f + at + 4, 4);
        if (n > kPngMaxChunk || n > len - at - 12 || len - at < 12)
            return snprintf(msg, msg_cap, "truncated chunk at offset %lld", (long long)at), false;
        if (first != (type == kPngIHDR)) return snprintf(msg, msg_cap, first ? "IHDR is not the first chunk" : "a second IHDR at offset %lld", (long long)at), false;
        const bool critical = type == kPngIHDR || type == kPngPLTE || type == kPngIDAT || type == kPngIEND;
        if (critical && check_crc && crc32_bytes_slow(0, f + at + 4, (uint64_t)n + 4) != png_be32(f + at + 8 + n)) {
            char t[5] = {(char)f[at + 4], (char)f[at + 5], (char)f[at + 6], (char)f[at + 7], 0};
            return snprintf(msg, msg_cap, "CRC error in %s chunk at offset %lld", t, (long long)at), false;
        }
        if (first) {
            first = false;
            if (n != 13) return snprintf(msg, msg_cap, "IHDR holds %lld bytes, not 13", (long long)n), false;
            const uint8_t *h = f + at + 8;
            info->width = png_be32(h), info->height = png_be32(h + 4);
            info->bit_depth = h[8], info->color_type = h[9], info->interlace = h[12];
            if (info->width < 1 || info->width > 0x7FFFFFFF || info->height < 1 || info->height > 0x7FFFFFFF)
                return snprintf(msg, msg_cap, "IHDR: width or height outside 1 .. 2^31 - 1"), false;
            if (!png_color_ok(info->color_type, info->bit_depth))
                return snprintf(msg, msg_cap, "IHDR: color type %d with bit depth %d", info->color_type, info->bit_depth), false;
            if (h[10] != 0 || h[11] != 0 || h[12] > 1)
                return snprintf(msg, msg_cap, "IHDR: compression %d, filter %d, interlace %d", h[10], h[11], h[12]), false;
            info->bits_per_pixel = info->bit_depth * png_channels(info->color_type);
            const int64_t rb = (info->width * info->bits_per_pixel + 7) >> 3;
            info->pixel_bytes = rb > INT64_MAX / info->height ? INT64_MAX : info->height * rb;  // (saturates: 2^31 rows of 2^34 bytes)
        }
        if (type == kPngIDAT) {
            if (idat_done) return snprintf(msg, msg_cap, "IDAT chunks are not consecutive (offset %lld)", (long long)at), false;
            in_idat = true;
            info->n_idat++, info->idat_bytes += n;
        } else if (in_idat)
            in_idat = false, idat_done = true;
        if (critical) emit(PngChunkRef{type, at, n});
        at += 12 + n;
        if (type == kPngIEND) {
            ended = true;
            break;  // (bytes behind IEND are not the file's)
        }
    }
    if (first) return snprintf(msg, msg_cap, "IHDR is missing"), false;
    if (info->n_idat == 0) return snprintf(msg, msg_cap, "no IDAT chunk"), false;
    if (!ended) return snprintf(msg, msg_cap, "IEND is missing"), false;
    return true;
}

// What a file says about its colours: the data bytes of its PLTE and tRNS chunks (0 entries / 0 bytes: none, or ignored).
struct PngFileColors {
    uint8_t plte[768], trns[256];
    int plte_entries, trns_len;
};
constexpr uint32_t kPngtRNS = png_type('t', 'R', 'N', 'S');
// The second walk, over a chain png_walk_file has accepted (`info` is its result): captures PLTE and tRNS, the one ancillary
// chunk that is interpreted -- so its CRC is checked, here on the host (it holds at most 256 bytes).  False with the reason
// in msg for: a PLTE whose length is no multiple of 3 or outside 3 .. 768, a second PLTE or tRNS, either of them behind the
// first IDAT, a type-3 file without a PLTE in front of its IDAT, a tRNS in front of the PLTE of a type-3 file, a tRNS whose
// length is not 2 (type 0), 6 (type 2) or 1 .. the PLTE's entries (type 3), a tRNS with a wrong CRC.  A tRNS of a type 4 or
// 6 file and a PLTE of a type 0 or 4 file are stepped over like any other chunk.
inline bool png_file_colors(const uint8_t *f, int64_t len, const PngFileInfo &info, PngFileColors *col, char *msg, size_t msg_cap) {
    memset(col, 0, sizeof *col);
    const int ct = info.color_type;
    const bool plte_counts = ct != 0 && ct != 4, trns_counts = ct != 4 && ct != 6;
    bool have_plte = false, have_trns = false, idat_seen = false;
    for (int64_t at = 8; at + 12 <= len;) {
        const int64_t n = png_be32(f + at);
        uint32_t type;
        memcpy(&type, f + at + 4, 4);
        if (type == kPngIDAT) idat_seen = true;
        if (type == kPngPLTE && plte_counts) {
            if (have_plte) return snprintf(msg, msg_cap, "a second PLTE at offset %lld", (long long)at), false;
            if (idat_seen) return snprintf(msg, msg_cap, "PLTE behind IDAT (offset %lld)", (long long)at), false;
            if (n % 3 != 0 || n < 3 || n > 768) return snprintf(msg, msg_cap, "PLTE holds %lld bytes", (long long)n), false;
            have_plte = true;
            col->plte_entries = (int)(n / 3);
            memcpy(col->plte, f + at + 8, (size_t)n);
        }
        if (type == kPngtRNS && trns_counts) {
            if (have_trns) return snprintf(msg, msg_cap, "a second tRNS at offset %lld", (long long)at), false;
            if (idat_seen) return snprintf(msg, msg_cap, "tRNS behind IDAT (offset %lld)", (long long)at), false;
            if (ct == 3 && !have_plte) return snprintf(msg, msg_cap, "tRNS in front of PLTE (offset %lld)", (long long)at), false;
            const bool fits = ct == 0 ? n == 2 : ct == 2 ? n == 6 : n >= 1 && n <= col->plte_entries;
            if (!fits) return snprintf(msg, msg_cap, "tRNS holds %lld bytes at color type %d", (long long)n, ct), false;
            if (crc32_bytes_slow(0, f + at + 4, (uint64_t)n + 4) != png_be32(f + at + 8 + n))
                return snprintf(msg, msg_cap, "CRC error in tRNS chunk at offset %lld", (long long)at), false;
            have_trns = true;
            col->trns_len = (int)n;
            memcpy(col->trns, f + at + 8, (size_t)n);
        }
        at += 12 + n;
        if (type == kPngIEND) break;
    }
    if (ct == 3 && !have_plte) return snprintf(msg, msg_cap, "color type 3 without a PLTE in front of IDAT"), false;
    return true;
}

// ---- animated PNG (APNG specification 1.0: acTL, fcTL, fdAT) ----
// One frame of an animation.  Mirrors zs_png_frame of the C ABI field for field (zs_engine.hip asserts it).
struct PngFrame {
    int64_t x, y, width, height;
    int delay_num, delay_den;
    int dispose_op, blend_op;
    int64_t data_bytes, n_chunks;
};
// What the animation walk finds in one file.  Mirrors zs_png_anim.
struct PngAnimInfo {
    PngFileInfo png;
    int animated;
    int n_frames, n_plays;
    int default_is_frame;
};
constexpr uint32_t kPngacTL = png_type('a', 'c', 'T', 'L'), kPngfcTL = png_type('f', 'c', 'T', 'L'), kPngfdAT = png_type('f', 'd', 'A', 'T');
constexpr int kPngDisposeNone = 0, kPngDisposeBackground = 1, kPngDisposePrevious = 2, kPngBlendSource = 0, kPngBlendOver = 1;

// The third walk, over a chain png_walk_file and png_file_colors have accepted (`info` is the first one's result): the
// animation.  A file without an acTL is an animation of one frame -- the whole canvas, dispose NONE, blend SOURCE, its data
// the IDAT stream -- and any fcTL / fdAT it holds is stepped over like other ancillary chunks.  With an acTL, the fcTL and
// fdAT chunks are interpreted: acTL and fcTL are verified here on the host (they hold 8 and 26 bytes); the fdAT CRCs are left
// to the device with the IDAT ones.  False with the reason in msg for: a second acTL, one that does not hold 8 bytes, one
// behind the first IDAT, num_frames 0 or above 2^31 - 1; an fcTL that does not hold 26 bytes, whose sequence number is not
// the next one (fcTL and fdAT share one counter from 0), a second one in front of IDAT, one in front of IDAT that is not
// the canvas at (0, 0), one without frame data behind it, one with width or height 0, a region beyond the canvas, dispose
// above 2 or blend above 1; an fdAT shorter than 4 bytes, with the wrong sequence number, in front of IDAT, or with no fcTL
// since IDAT; a number of fcTLs other than num_frames; a wrong CRC in acTL or fcTL.
// emit_frame(k, frame) is called once per frame, in order, when its last data chunk has been seen; emit_data(k, ref) for
// every chunk that holds data of frame k (IDAT: ref.len bytes at ref.at + 8; fdAT: ref.len - 4 bytes at ref.at + 12).
template <class EmitFrame, class EmitData>
inline bool png_walk_anim(const uint8_t *f, int64_t len, const PngFileInfo &info, PngAnimInfo *anim, char *msg, size_t msg_cap, EmitFrame emit_frame,
                          EmitData emit_data) {
    anim->png = info;
    anim->animated = 0, anim->n_frames = 1, anim->n_plays = 0, anim->default_is_frame = 1;
    for (int64_t at = 8; at + 12 <= len;) {  // is there an acTL at all?
        const int64_t n = png_be32(f + at);
        uint32_t type;
        memcpy(&type, f + at + 4, 4);
        if (type == kPngacTL) anim->animated = 1;
        at += 12 + n;
        if (type == kPngIEND) break;
    }
    PngFrame cur;
    memset(&cur, 0, sizeof cur);
    if (!anim->animated) {
        cur.width = info.width, cur.height = info.height;
        cur.dispose_op = kPngDisposeNone, cur.blend_op = kPngBlendSource;
        for (int64_t at = 8; at + 12 <= len;) {
            const int64_t n = png_be32(f + at);
            uint32_t type;
            memcpy(&type, f + at + 4, 4);
            if (type == kPngIDAT) {
                cur.data_bytes += n, cur.n_chunks++;
                emit_data(0, PngChunkRef{type, at, n});
            }
            at += 12 + n;
            if (type == kPngIEND) break;
        }
        emit_frame(0, cur);
        return true;
    }
    auto crc_ok = [&](int64_t at, int64_t n) { return crc32_bytes_slow(0, f + at + 4, (uint64_t)n + 4) == png_be32(f + at + 8 + n); };
    bool have_actl = false, idat_seen = false, open = false;  // open: an fcTL whose frame has not been emitted yet
    int64_t num_frames = 0, n_fctl = 0;
    uint32_t seq = 0;
    int fctl_before_idat = 0;
    anim->default_is_frame = 0;
    auto close = [&](int64_t at) {  // the open frame ends in front of the chunk at `at`
        if (!open) return true;
        if (cur.n_chunks == 0) return snprintf(msg, msg_cap, "fcTL of frame %lld has no frame data (offset %lld)", (long long)(n_fctl - 1), (long long)at), false;
        emit_frame((int)(n_fctl - 1), cur);
        open = false;
        return true;
    };
    for (int64_t at = 8; at + 12 <= len;) {
        const int64_t n = png_be32(f + at);
        uint32_t type;
        memcpy(&type, f + at + 4, 4);
        const uint8_t *d = f + at + 8;
        if (type == kPngacTL) {
            if (have_actl) return snprintf(msg, msg_cap, "a second acTL at offset %lld", (long long)at), false;
            if (idat_seen) return snprintf(msg, msg_cap, "acTL behind IDAT (offset %lld)", (long long)at), false;
            if (n != 8) return snprintf(msg, msg_cap, "acTL holds %lld bytes, not 8", (long long)n), false;
            if (!crc_ok(at, n)) return snprintf(msg, msg_cap, "CRC error in acTL chunk at offset %lld", (long long)at), false;
            have_actl = true;
            num_frames = png_be32(d);
            if (num_frames < 1 || num_frames > 0x7FFFFFFF) return snprintf(msg, msg_cap, "acTL: num_frames outside 1 .. 2^31 - 1"), false;
            anim->n_frames = (int)num_frames, anim->n_plays = (int)(png_be32(d + 4) & 0x7FFFFFFFu);
        } else if (type == kPngfcTL) {
            if (n != 26) return snprintf(msg, msg_cap, "fcTL holds %lld bytes, not 26 (offset %lld)", (long long)n, (long long)at), false;
            if (!crc_ok(at, n)) return snprintf(msg, msg_cap, "CRC error in fcTL chunk at offset %lld (frame %lld)", (long long)at, (long long)n_fctl), false;
            if (png_be32(d) != seq)
                return snprintf(msg, msg_cap, "fcTL at offset %lld has sequence number %u, not %u", (long long)at, png_be32(d), seq), false;
            seq++;
            if (!idat_seen && ++fctl_before_idat > 1) return snprintf(msg, msg_cap, "a second fcTL in front of IDAT (offset %lld)", (long long)at), false;
            if (!close(at)) return false;
            memset(&cur, 0, sizeof cur);
            cur.width = png_be32(d + 4), cur.height = png_be32(d + 8), cur.x = png_be32(d + 12), cur.y = png_be32(d + 16);
            cur.delay_num = d[20] << 8 | d[21], cur.delay_den = d[22] << 8 | d[23];
            cur.dispose_op = d[24], cur.blend_op = d[25];
            if (cur.width < 1 || cur.height < 1) return snprintf(msg, msg_cap, "fcTL of frame %lld: width or height 0", (long long)n_fctl), false;
            if (cur.x + cur.width > info.width || cur.y + cur.height > info.height)
                return snprintf(msg, msg_cap, "fcTL of frame %lld: the region reaches beyond the canvas", (long long)n_fctl), false;
            if (cur.dispose_op > 2 || cur.blend_op > 1)
                return snprintf(msg, msg_cap, "fcTL of frame %lld: dispose %d, blend %d", (long long)n_fctl, cur.dispose_op, cur.blend_op), false;
            if (!idat_seen && (cur.x != 0 || cur.y != 0 || cur.width != info.width || cur.height != info.height))
                return snprintf(msg, msg_cap, "the fcTL in front of IDAT is not the whole canvas"), false;
            if (!idat_seen) anim->default_is_frame = 1;
            open = true;
            n_fctl++;
        } else if (type == kPngIDAT) {
            idat_seen = true;
            if (anim->default_is_frame) {
                cur.data_bytes += n, cur.n_chunks++;
                emit_data(0, PngChunkRef{type, at, n});
            }
        } else if (type == kPngfdAT) {
            if (n < 4) return snprintf(msg, msg_cap, "fdAT holds %lld bytes (offset %lld)", (long long)n, (long long)at), false;
            if (!idat_seen) return snprintf(msg, msg_cap, "fdAT in front of IDAT (offset %lld)", (long long)at), false;
            if (n_fctl - fctl_before_idat < 1) return snprintf(msg, msg_cap, "fdAT without an fcTL since IDAT (offset %lld)", (long long)at), false;
            if (png_be32(d) != seq)
                return snprintf(msg, msg_cap, "fdAT at offset %lld has sequence number %u, not %u", (long long)at, png_be32(d), seq), false;
            seq++;
            cur.data_bytes += n - 4, cur.n_chunks++;
            emit_data((int)(n_fctl - 1), PngChunkRef{type, at, n});
        }
        at += 12 + n;
        if (type == kPngIEND) {
            if (!close(at - 12 - n)) return false;
            break;
        }
    }
    if (n_fctl != num_frames) return snprintf(msg, msg_cap, "acTL announces %lld frames, the file has %lld fcTL chunks", (long long)num_frames, (long long)n_fctl), false;
    return true;
}

}  // namespace zs
