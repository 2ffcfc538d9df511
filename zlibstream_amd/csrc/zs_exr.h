// zs_exr.h -- the OpenEXR container with ZIP / ZIPS compression as far as this library reads and writes it: the rules by which
// the host walks a file's header, offset table and chunk headers (zs_exr_host.inc, zs_exr_file_info and
// zs_exr_decode_files_batch), the bytes the writer puts around the chunks (zs_exr_encode_batch_device), and the per-lane step
// of the predictor kernels (KE, zs_exr.hip); tests/cpp/test_exr_walk.cpp runs them on the host.  Nothing here reads outside
// [file, file + len).  include/zsgpu.h states the rules in full; no third-party reader was at hand to check them against.
//
// A file:  76 2F 31 01, a version word (low byte 2; 0x200 tiled, 0x400 long names)
//          the header: attributes [name\0 type\0 int32 size, size bytes], a \0 ends them
//          the offset table: one uint64 per chunk, in the order of the chunks' places whatever the line order
//          the chunks: [int32 y | int32 tileX, tileY, levelX, levelY] int32 dataSize, data
// A chunk's raw bytes: for each row, for each channel in the list's order, its w samples.  dataSize == their count: they lie
// raw; less: a zlib stream of them predicted -- split into the bytes at even and at odd places, then differenced as one run.
#pragma once

#include <cstdint>

#include "zs_core.h"

namespace zs {

constexpr int64_t kExrMaxLen = 0x7FFFFFFF - 1024;  // a file and an image's planes, in one call of the engine
constexpr int kExrMaxChannels = 64;
constexpr int kExrTile = 32 << 10;     // output bytes of one tile of KE: one wave's work
constexpr int kExrSeg = kExrTile / 2;  // ... which are that many bytes of each half of the chunk's stored bytes
constexpr int kExrPass = 64 * 16;      // bytes of each half that one pass of the wave takes

enum ExrErr {
    kExrOk = 0,
    kExrShortFile, kExrBadMagic, kExrBadVersion, kExrDeep, kExrMultiPart, kExrBadFlags, kExrHeaderOut, kExrLongName, kExrBadAttr, kExrMissing,
    kExrBadWindow, kExrNoChannels, kExrManyChannels, kExrBadType, kExrBadSampling, kExrBadCompression, kExrBadLevels, kExrBadTile, kExrBadOrder,
    kExrTableOut, kExrTooLarge,            // the file
    kExrTruncated, kExrBadPlace, kExrBadSize  // a chunk
};
ZS_HD int exr_err_status(int e) { return e == kExrOk ? 0 : (e == kExrShortFile || e == kExrTruncated) ? -5 : -3; }
inline const char *exr_err_message(int e) {
    switch (e) {
    case kExrOk: return "";
    case kExrBadMagic: return "not an OpenEXR file";
    case kExrBadVersion: return "unsupported file version";
    case kExrDeep: return "deep data is not supported";
    case kExrMultiPart: return "multi-part files are not supported";
    case kExrBadFlags: return "unsupported version flags";
    case kExrHeaderOut: return "the header reaches out of the file";
    case kExrLongName: return "a name is longer than the version flags allow";
    case kExrBadAttr: return "an attribute's size disagrees with its type";
    case kExrMissing: return "a required attribute is missing";
    case kExrBadWindow: return "invalid data window";
    case kExrNoChannels: return "no channels";
    case kExrManyChannels: return "more than 64 channels";
    case kExrBadType: return "unsupported pixel type";
    case kExrBadSampling: return "unsupported channel sampling";
    case kExrBadCompression: return "unsupported compression method";
    case kExrBadLevels: return "unsupported level mode";
    case kExrBadTile: return "invalid tile size";
    case kExrBadOrder: return "random line order in a scanline file";
    case kExrTableOut: return "the offset table reaches out of the file";
    case kExrTooLarge: return "the image is above 2 GiB - 1 KiB";
    case kExrBadPlace: return "a chunk's coordinates do not match its place";
    case kExrBadSize: return "invalid chunk size";
    default: return "buffer error";
    }
}

// the three structs of include/zsgpu.h (zs_exr_info, zs_exr_channel, zs_exr_chunk), field for field
struct ExrInfo {
    int32_t data_window[4], display_window[4];  // xMin, yMin, xMax, yMax
    int64_t width, height;
    int n_channels, compression, line_order, tiled;
    int has_display_window, long_names;
    int64_t tile_w, tile_h;
    int64_t lines_per_chunk, n_chunks, out_len;
};
struct ExrChannel {
    char name[256];
    int type, sample_bytes;
    int64_t plane_off;
};
struct ExrChunk {
    int64_t off, data_len, raw_len;  // the data behind the chunk's header; how many bytes they stand for
    int64_t x, y, w, h;              // its place in the data window, counted from the window's corner
    int status, reason;              // the library's code, and the ExrErr behind it
};

ZS_HD uint32_t exr_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
ZS_HD int32_t exr_i32(const uint8_t *p) { return (int32_t)exr_u32(p); }
ZS_HD uint64_t exr_u64(const uint8_t *p) { return (uint64_t)exr_u32(p) | (uint64_t)exr_u32(p + 4) << 32; }
ZS_HD void exr_put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24); }
ZS_HD void exr_put64(uint8_t *p, uint64_t v) { exr_put32(p, (uint32_t)v), exr_put32(p + 4, (uint32_t)(v >> 32)); }
ZS_HD int64_t exr_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
ZS_HD int exr_type_bytes(int type) { return type == 1 ? 2 : 4; }
ZS_HD int exr_lines(int compression) { return compression == 3 ? 16 : 1; }

// the string at f[at ..): its length, -1 where the file ends in front of its \0
inline int64_t exr_strlen(const uint8_t *f, int64_t at, int64_t end) {
    for (int64_t i = at; i < end; i++)
        if (f[i] == 0) return i - at;
    return -1;
}
inline bool exr_is(const uint8_t *f, int64_t at, int64_t n, const char *s) {
    int64_t k = 0;
    while (s[k]) k++;
    if (k != n) return false;
    for (int64_t i = 0; i < n; i++)
        if (f[at + i] != (uint8_t)s[i]) return false;
    return true;
}

// The whole walk.  kExrOk and *info; the first ch_cap channels in ch[] and the first `cap` chunks in chunks[] (either may be
// null with its cap 0), each chunk with status 0 or the library's code for what is wrong with it alone.  Otherwise the file's
// error, with *info as far as the walk got.
inline int exr_walk(const uint8_t *f, int64_t len, ExrInfo *info, ExrChannel *ch, int64_t ch_cap, ExrChunk *chunks, int64_t cap) {
    *info = ExrInfo{};
    if (len < 8) return kExrShortFile;
    if (!(f[0] == 0x76 && f[1] == 0x2F && f[2] == 0x31 && f[3] == 0x01)) return kExrBadMagic;
    const uint32_t version = exr_u32(f + 4);
    if ((version & 0xFF) != 2) return kExrBadVersion;
    if (version & 0x800) return kExrDeep;
    if (version & 0x1000) return kExrMultiPart;
    if (version & ~(uint32_t)0x6FF) return kExrBadFlags;
    const bool tiled = (version & 0x200) != 0;
    const int64_t max_name = (version & 0x400) ? 255 : 31;
    info->tiled = tiled, info->long_names = (version & 0x400) != 0;
    // ---- the attributes
    int64_t at = 8, chlist_at = -1, chlist_len = 0;
    bool has_compression = false, has_window = false, has_order = false, has_tiles = false;
    uint32_t tile_w = 0, tile_h = 0;
    int tile_mode = 0;
    for (;;) {
        if (at >= len) return kExrHeaderOut;
        if (f[at] == 0) {
            at++;
            break;
        }
        const int64_t n_name = exr_strlen(f, at, len);
        if (n_name < 0) return kExrHeaderOut;
        if (n_name > max_name) return kExrLongName;
        const int64_t type_at = at + n_name + 1, n_type = exr_strlen(f, type_at, len);
        if (n_type < 0) return kExrHeaderOut;
        if (n_type > max_name) return kExrLongName;
        const int64_t size_at = type_at + n_type + 1;
        if (len - size_at < 4) return kExrHeaderOut;
        const int32_t size = exr_i32(f + size_at);
        const int64_t v = size_at + 4;
        if (size < 0 || size > len - v) return kExrHeaderOut;
        auto named = [&](const char *name) { return exr_is(f, at, n_name, name); };
        auto typed = [&](const char *type, int32_t bytes) { return exr_is(f, type_at, n_type, type) && (bytes < 0 ? size >= 1 : size == bytes); };
        if (named("channels")) {
            if (!typed("chlist", -1)) return kExrBadAttr;
            chlist_at = v, chlist_len = size;
        } else if (named("compression")) {
            if (!typed("compression", 1)) return kExrBadAttr;
            info->compression = f[v], has_compression = true;
        } else if (named("dataWindow")) {
            if (!typed("box2i", 16)) return kExrBadAttr;
            for (int k = 0; k < 4; k++) info->data_window[k] = exr_i32(f + v + 4 * k);
            has_window = true;
        } else if (named("lineOrder")) {
            if (!typed("lineOrder", 1)) return kExrBadAttr;
            info->line_order = f[v], has_order = true;
        } else if (named("tiles") && tiled) {
            if (!typed("tiledesc", 9)) return kExrBadAttr;
            tile_w = exr_u32(f + v), tile_h = exr_u32(f + v + 4), tile_mode = f[v + 8], has_tiles = true;
        } else if (named("displayWindow") && typed("box2i", 16)) {
            for (int k = 0; k < 4; k++) info->display_window[k] = exr_i32(f + v + 4 * k);
            info->has_display_window = 1;
        }
        at = v + size;
    }
    if (chlist_at < 0 || !has_compression || !has_window || !has_order || (tiled && !has_tiles)) return kExrMissing;
    const int64_t x_min = info->data_window[0], y_min = info->data_window[1], x_max = info->data_window[2], y_max = info->data_window[3];
    if (x_max < x_min || y_max < y_min) return kExrBadWindow;
    const int64_t W = x_max - x_min + 1, H = y_max - y_min + 1;  // (below 2^32)
    info->width = W, info->height = H;
    // ---- the channels, inside their attribute
    int types[kExrMaxChannels];
    int n_ch = 0;
    {
        const int64_t end = chlist_at + chlist_len;
        int64_t p = chlist_at;
        for (;;) {
            if (p >= end) return kExrBadAttr;
            if (f[p] == 0) break;
            const int64_t n_name = exr_strlen(f, p, end);
            if (n_name < 0) return kExrBadAttr;
            if (n_name > max_name) return kExrLongName;
            if (end - (p + n_name + 1) < 16) return kExrBadAttr;
            if (n_ch == kExrMaxChannels) return kExrManyChannels;
            const uint8_t *q = f + p + n_name + 1;
            const uint32_t type = exr_u32(q);
            if (type > 2) return kExrBadType;
            if (exr_i32(q + 8) != 1 || exr_i32(q + 12) != 1) return kExrBadSampling;
            types[n_ch] = (int)type;
            if (n_ch < ch_cap) {
                ExrChannel &c = ch[n_ch];
                for (int64_t k = 0; k < 256; k++) c.name[k] = k < n_name ? (char)f[p + k] : 0;
                c.type = (int)type, c.sample_bytes = exr_type_bytes((int)type), c.plane_off = 0;
            }
            n_ch++;
            p += n_name + 1 + 16;
        }
    }
    if (n_ch == 0) return kExrNoChannels;
    info->n_channels = n_ch;
    if (!(info->compression == 0 || info->compression == 2 || info->compression == 3)) return kExrBadCompression;
    if (info->line_order > 2) return kExrBadOrder;
    if (tiled) {
        if ((tile_mode & 15) != 0) return kExrBadLevels;
        if (tile_w < 1 || tile_h < 1 || tile_w > 0x7FFFFFFFu || tile_h > 0x7FFFFFFFu) return kExrBadTile;
        info->tile_w = tile_w, info->tile_h = tile_h;
    } else if (info->line_order == 2) {
        return kExrBadOrder;
    }
    // ---- the planes: plane c is H rows of W samples, at the running sum rounded up to 16
    if (W > kExrMaxLen / H) return kExrTooLarge;
    int64_t bpp = 0, end = 0;
    for (int c = 0; c < n_ch; c++) {
        const int64_t off = (end + 15) & ~(int64_t)15, bytes = W * H * exr_type_bytes(types[c]);  // (below 2^33)
        if (off + bytes > kExrMaxLen) return kExrTooLarge;
        if (c < ch_cap) ch[c].plane_off = off;
        end = off + bytes, bpp += exr_type_bytes(types[c]);
    }
    info->out_len = end;
    // ---- the offset table
    const int64_t L = tiled ? (int64_t)tile_h : exr_lines(info->compression);
    const int64_t cw = tiled ? (int64_t)tile_w : W, nx = exr_ceil_div(W, cw), ny = exr_ceil_div(H, L);
    info->lines_per_chunk = L, info->n_chunks = nx * ny;  // (at most W * H)
    if (info->n_chunks > (len - at) / 8) return kExrTableOut;
    const int64_t head = tiled ? 20 : 8;
    for (int64_t k = 0; k < info->n_chunks && k < cap; k++) {
        ExrChunk c{};
        c.x = (k % nx) * cw, c.y = (k / nx) * L;
        c.w = W - c.x < cw ? W - c.x : cw, c.h = H - c.y < L ? H - c.y : L;
        c.raw_len = c.w * c.h * bpp;
        const uint64_t off = exr_u64(f + at + 8 * k);
        int why = kExrOk;
        if (off > (uint64_t)len || len - (int64_t)off < head) {
            why = kExrTruncated;
        } else {
            const uint8_t *p = f + off;
            const bool here = tiled ? exr_i32(p) == k % nx && exr_i32(p + 4) == k / nx && exr_i32(p + 8) == 0 && exr_i32(p + 12) == 0 : (int64_t)exr_i32(p) == y_min + c.y;
            const int64_t size = exr_i32(p + head - 4);
            if (!here) why = kExrBadPlace;
            else if (size < 0 || size > c.raw_len) why = kExrBadSize;
            else if (len - (int64_t)off - head < size) why = kExrTruncated;
            else c.off = (int64_t)off + head, c.data_len = size;
        }
        c.status = exr_err_status(why), c.reason = why;
        chunks[k] = c;
    }
    return kExrOk;
}

// ---- the writer: a single-part scanline file, increasing Y, [magic, version 2 | the attributes | the offset table | the chunks]
struct ExrLayout {
    int64_t width, height;
    int32_t x_min, y_min;
    int n_channels, compression;
    const char *const *names;
    const int *types;
    const uint8_t *extra;  // attributes the caller has encoded, copied as they are
    int64_t extra_len;
    int64_t bpp, n_chunks;
};
ZS_HD int64_t exr_strlen0(const char *s) {
    int64_t k = 0;
    while (s[k]) k++;
    return k;
}
// bytes in front of the first chunk
inline int64_t exr_head_bytes(const ExrLayout &l) {
    int64_t chl = 1;
    for (int c = 0; c < l.n_channels; c++) chl += exr_strlen0(l.names[c]) + 1 + 16;
    const int64_t attrs = (9 + 7 + 4 + chl) + (12 + 12 + 4 + 1) + (11 + 6 + 4 + 16) + (14 + 6 + 4 + 16) + (10 + 10 + 4 + 1) + (17 + 6 + 4 + 4) + (19 + 4 + 4 + 8) +
                          (18 + 6 + 4 + 4);
    return 8 + attrs + l.extra_len + 1 + 8 * l.n_chunks;
}
// The head into p[0 .. exr_head_bytes): body_len[k] is what chunk k's data take; chunk k's 8-byte header lies at chunk_off[k]
// (written here), its data behind it.  Returns the file's length.
inline int64_t exr_put_head(uint8_t *p, const ExrLayout &l, const int64_t *body_len, int64_t *chunk_off) {
    uint8_t *q = p;
    auto str = [&](const char *s) {
        do *q++ = (uint8_t)*s;
        while (*s++);
    };
    auto attr = [&](const char *name, const char *type, int64_t size) { str(name), str(type), exr_put32(q, (uint32_t)size), q += 4; };
    auto u32 = [&](uint32_t v) { exr_put32(q, v), q += 4; };
    *q++ = 0x76, *q++ = 0x2F, *q++ = 0x31, *q++ = 0x01;
    u32(2);
    int64_t chl = 1;
    for (int c = 0; c < l.n_channels; c++) chl += exr_strlen0(l.names[c]) + 1 + 16;
    attr("channels", "chlist", chl);
    for (int c = 0; c < l.n_channels; c++) str(l.names[c]), u32((uint32_t)l.types[c]), u32(0), u32(1), u32(1);
    *q++ = 0;
    attr("compression", "compression", 1), *q++ = (uint8_t)l.compression;
    for (int twice = 0; twice < 2; twice++) {
        attr(twice ? "displayWindow" : "dataWindow", "box2i", 16);
        u32((uint32_t)l.x_min), u32((uint32_t)l.y_min), u32((uint32_t)(l.x_min + (int32_t)(l.width - 1))), u32((uint32_t)(l.y_min + (int32_t)(l.height - 1)));
    }
    attr("lineOrder", "lineOrder", 1), *q++ = 0;
    attr("pixelAspectRatio", "float", 4), u32(0x3F800000u);
    attr("screenWindowCenter", "v2f", 8), u32(0), u32(0);
    attr("screenWindowWidth", "float", 4), u32(0x3F800000u);
    for (int64_t i = 0; i < l.extra_len; i++) *q++ = l.extra[i];
    *q++ = 0;
    int64_t at = (q - p) + 8 * l.n_chunks;
    for (int64_t k = 0; k < l.n_chunks; k++) {
        exr_put64(q, (uint64_t)at), q += 8;
        chunk_off[k] = at;
        at += 8 + body_len[k];
    }
    return at;
}

// ---- the predictor kernels' per-lane step (KE, zs_exr.hip; tests/cpp/test_exr_walk.cpp runs the same code over a model of
// the wave).  The stored bytes t[0, U) are two halves, [0, h) and [h, U) with h = (U + 1) / 2.  The undo is
//   t'[i] = t[0] + .. + t[i] - 128 i  (mod 256)      raw[2 k] = t'[k], raw[2 k + 1] = t'[h + k]
// and 128 i mod 256 is 128 for odd i, else 0: a flip of the top bit.  A lane holds bytes [a, a + 16) of each half, a a
// multiple of 16, as four little-endian words each, and all sums are done on the packed bytes.

// a + b and a - b per byte, mod 256: the top bits are kept out of the word's carries and put back by the xor
ZS_HD uint32_t exr_add8(uint32_t a, uint32_t b) { return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u); }
ZS_HD uint32_t exr_sub8(uint32_t a, uint32_t b) { return ((a | 0x80808080u) - (b & 0x7F7F7F7Fu)) ^ ((a ^ ~b) & 0x80808080u); }
// the sum of a word's four bytes, in its low byte (the rest is to be masked away)
ZS_HD uint32_t exr_fold8(uint32_t x) { return x + (x >> 8) + (x >> 16) + (x >> 24); }
// the four bytes of the group's byte sum (for the reduce launch: only their total counts)
ZS_HD uint32_t exr_group_sum(const uint32_t w[4]) { return exr_add8(exr_add8(w[0], w[1]), exr_add8(w[2], w[3])); }
// every byte becomes the sum of the group's bytes up to it; returns the last one, the group's total (low byte)
ZS_HD uint32_t exr_lane_scan(uint32_t w[4]) {
    uint32_t carry = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t x = w[k];
        x = exr_add8(x, x << 8);
        x = exr_add8(x, x << 16);
        x = exr_add8(x, carry * 0x01010101u);
        w[k] = x, carry = x >> 24;
    }
    return carry;
}
// `add` (a byte: what lies in front of the group) onto every byte, then the flip of the bytes at odd places of the chunk:
// odd = 1 where the group's first byte lies at an odd place
ZS_HD void exr_lane_finish(uint32_t w[4], uint32_t add, int odd) {
    const uint32_t a = (add & 0xFF) * 0x01010101u, flip = odd ? 0x00800080u : 0x80008000u;
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = exr_add8(w[k], a) ^ flip;
}
// bytes 0 and 1 of x to bytes 0 and 2
ZS_HD uint32_t exr_spread(uint32_t x) { return (x & 0xFF) | ((x & 0xFF00) << 8); }
ZS_HD uint32_t exr_gather(uint32_t x) { return (x & 0xFF) | ((x >> 8) & 0xFF00); }
// raw[2 k] = a[k], raw[2 k + 1] = b[k] for the group's 16 places, and back
ZS_HD void exr_interleave(const uint32_t a[4], const uint32_t b[4], uint32_t raw[8]) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        raw[2 * k] = exr_spread(a[k]) | exr_spread(b[k]) << 8;
        raw[2 * k + 1] = exr_spread(a[k] >> 16) | exr_spread(b[k] >> 16) << 8;
    }
}
ZS_HD void exr_split(const uint32_t raw[8], uint32_t a[4], uint32_t b[4]) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        a[k] = exr_gather(raw[2 * k]) | exr_gather(raw[2 * k + 1]) << 16;
        b[k] = exr_gather(raw[2 * k] >> 8) | exr_gather(raw[2 * k + 1] >> 8) << 16;
    }
}
// the forward step: every byte minus the one in front of it plus 128; `prev` is the byte in front of the group (128 in front
// of the chunk's first byte, which is stored as it is)
ZS_HD void exr_lane_diff(uint32_t w[4], uint32_t prev) {
    uint32_t before = prev & 0xFF;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t x = w[k];
        w[k] = exr_sub8(x, x << 8 | before) ^ 0x80808080u;
        before = x >> 24;
    }
}

// One run of a chunk's raw bytes: bytes [off, off + len) lie at p -- one (row, channel) of a plane; the contiguous calls have
// one run for all.  A chunk's runs are ascending and without gaps from 0 to its length.
struct ExrRun {
    uint8_t *p;
    int32_t off, len;
};
// One chunk of a KE launch, either direction.
struct ExrJob {
    uint8_t *t;       // the stored bytes: read by the undo, written by the forward kernel
    int32_t len;      // U
    int32_t run0, n_runs;
    int32_t plain;    // both steps off: the stored bytes are the raw bytes
};
ZS_HD int64_t exr_tiles(int64_t len) { return (((len + 1) >> 1) + kExrSeg - 1) / kExrSeg; }
// the run that holds byte `pos` of the chunk: the last one that begins at or in front of it
ZS_HD int exr_find_run(const ExrRun *runs, int n, int64_t pos) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (runs[mid].off <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace zs
