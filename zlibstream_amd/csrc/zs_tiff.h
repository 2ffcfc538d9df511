// zs_tiff.h -- the TIFF container (TIFF 6.0, Adobe's technical note on the Deflate compression, the BigTIFF layout) as far as
// this library reads and writes it: the rules by which the host walks a file's IFD chain and places every strip or tile
// (zs_tiff_host.inc, zs_tiff_file_info and zs_tiff_decode_files_batch), the bytes the writer puts around the chunks
// (zs_tiff_encode_batch_device), and the per-lane step of the predictor kernels (KT, zs_tiff.hip);
// tests/cpp/test_tiff_walk.cpp runs them on the host.  Nothing here reads outside [file, file + len).
//
// A file:  header (8: "II" or "MM", 42, the first IFD's offset; BigTIFF 16: 43, 8, 0, a 64-bit offset)
//          IFD: entry count (2; BigTIFF 8), entries of 12 (20) bytes [tag, type, count, value or offset], the next IFD's offset
//          a value longer than 4 (8) bytes lies where its entry's offset says
// All numbers in the byte order the header names.  A page is one IFD of the chain; SubIFDs are not followed.
// A chunk is a strip (all columns, RowsPerStrip rows) or a tile (TileWidth x TileLength, a whole tile even where it hangs
// over the image's right or bottom edge); with compression 8 or 32946 each chunk is a zlib stream of its own.
#pragma once

#include <cstdint>

#include "zs_core.h"

namespace zs {

constexpr int64_t kTiffMaxLen = 0x7FFFFFFF - 1024;  // a file and a page's pixels, in one call of the engine
constexpr int kTiffMaxSpp = 8;

// what is wrong: with the file or the page (the walk ends) or with one chunk (the walk goes on)
enum TiffErr {
    kTiffOk = 0,
    kTiffShortFile, kTiffBadMagic, kTiffBadIfd, kTiffBadValue, kTiffLoop, kTiffNoPage, kTiffMissingTag, kTiffBadCount, kTiffBadDims,
    kTiffBadCompression, kTiffBadPredictor, kTiffBadPlanar, kTiffBadBits, kTiffBadSamples, kTiffBadFillOrder, kTiffYCbCr, kTiffBadChunkSize,
    kTiffTooLarge,   // the file
    kTiffTruncated   // a chunk
};
// the library's codes (include/zsgpu.h ZS_DATA_ERROR, ZS_BUF_ERROR) and messages of these
ZS_HD int tiff_err_status(int e) { return e == kTiffOk ? 0 : (e == kTiffShortFile || e == kTiffTruncated) ? -5 : -3; }
inline const char *tiff_err_message(int e) {
    switch (e) {
    case kTiffOk: return "";
    case kTiffBadMagic: return "not a TIFF file";
    case kTiffBadIfd: return "an IFD reaches out of the file";
    case kTiffBadValue: return "a tag's value reaches out of the file or has a type that cannot hold it";
    case kTiffLoop: return "the IFD chain loops";
    case kTiffNoPage: return "no such page";
    case kTiffMissingTag: return "a required tag is missing";
    case kTiffBadCount: return "the offsets or byte counts are not one per strip or tile";
    case kTiffBadDims: return "invalid image dimensions";
    case kTiffBadCompression: return "unsupported compression method";
    case kTiffBadPredictor: return "unsupported predictor";
    case kTiffBadPlanar: return "unsupported planar configuration";
    case kTiffBadBits: return "unsupported bits per sample";
    case kTiffBadSamples: return "unsupported samples per pixel";
    case kTiffBadFillOrder: return "unsupported fill order";
    case kTiffYCbCr: return "YCbCr images are not supported";
    case kTiffBadChunkSize: return "invalid strip or tile size";
    case kTiffTooLarge: return "the image is above 2 GiB - 1 KiB";
    default: return "buffer error";
    }
}

// the two structs of include/zsgpu.h (zs_tiff_info, zs_tiff_chunk), field for field
struct TiffInfo {
    int64_t n_pages;
    int big_endian, bigtiff;
    int64_t width, height;
    int bits, spp, sample_format, photometric;
    int extra_samples, extra_kind;  // how many, and the first one's kind (0 where there is none)
    int compression, predictor, planar, orientation;
    int tiled, pad;
    int64_t chunk_w, chunk_h, n_chunks;
    int64_t row_bytes, out_len;
};
struct TiffChunk {
    int64_t off, comp_len;
    int64_t x, y, w, h;  // its place in the image, and the part of it that lies inside
    int status, pad;
};

struct TiffOrder {
    bool be, big;
};
ZS_HD uint32_t tiff_u16(const uint8_t *p, bool be) { return be ? (uint32_t)p[0] << 8 | p[1] : (uint32_t)p[1] << 8 | p[0]; }
ZS_HD uint32_t tiff_u32(const uint8_t *p, bool be) { return be ? tiff_u16(p, true) << 16 | tiff_u16(p + 2, true) : tiff_u16(p + 2, false) << 16 | tiff_u16(p, false); }
ZS_HD uint64_t tiff_u64(const uint8_t *p, bool be) {
    return be ? (uint64_t)tiff_u32(p, true) << 32 | tiff_u32(p + 4, true) : (uint64_t)tiff_u32(p + 4, false) << 32 | tiff_u32(p, false);
}
ZS_HD int64_t tiff_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// bytes of one row of `width` pixels
ZS_HD int64_t tiff_row_bytes(int64_t width, int spp, int bits) { return (width * spp * bits + 7) / 8; }

// One IFD entry: where its `count` values of `type` lie.  Types that hold an unsigned number: BYTE 1, SHORT 3, LONG 4, LONG8 16
// (and IFD 13, IFD8 18, which some writers use for offsets).
struct TiffEntry {
    int tag, type;
    uint64_t count;
    int64_t at;  // the values' place in the file, all of them inside it; -1: the entry is absent
};
ZS_HD int tiff_type_bytes(int type) { return type == 1 ? 1 : type == 3 ? 2 : (type == 4 || type == 13) ? 4 : (type == 16 || type == 18) ? 8 : 0; }
ZS_HD uint64_t tiff_entry_value(const uint8_t *f, const TiffEntry &e, uint64_t k, bool be) {
    const uint8_t *p = f + e.at + (int64_t)k * tiff_type_bytes(e.type);
    switch (tiff_type_bytes(e.type)) {
    case 1: return p[0];
    case 2: return tiff_u16(p, be);
    case 4: return tiff_u32(p, be);
    default: return tiff_u64(p, be);
    }
}

// The header: the order, and the first IFD's offset.
ZS_HD int tiff_read_header(const uint8_t *f, int64_t len, TiffOrder *o, uint64_t *first) {
    if (len < 8) return kTiffShortFile;
    if (!((f[0] == 'I' && f[1] == 'I') || (f[0] == 'M' && f[1] == 'M'))) return kTiffBadMagic;
    o->be = f[0] == 'M';
    const uint32_t version = tiff_u16(f + 2, o->be);
    if (version == 42) {
        o->big = false, *first = tiff_u32(f + 4, o->be);
        return kTiffOk;
    }
    if (version != 43) return kTiffBadMagic;
    if (len < 16) return kTiffShortFile;
    if (tiff_u16(f + 4, o->be) != 8 || tiff_u16(f + 6, o->be) != 0) return kTiffBadMagic;
    o->big = true, *first = tiff_u64(f + 8, o->be);
    return kTiffOk;
}

// The IFD at `off`: its entry count and the next IFD's offset; kTiffBadIfd where it does not lie inside the file.
ZS_HD int tiff_read_ifd(const uint8_t *f, int64_t len, TiffOrder o, uint64_t off, uint64_t *n_entries, uint64_t *next) {
    const int64_t head = o.big ? 8 : 2, each = o.big ? 20 : 12, tail = o.big ? 8 : 4;
    if (off < 8 || off > (uint64_t)len || len - (int64_t)off < head) return kTiffBadIfd;
    const uint64_t n = o.big ? tiff_u64(f + off, o.be) : tiff_u16(f + off, o.be);
    const int64_t room = len - (int64_t)off - head;
    if (n > (uint64_t)(room / each) || room - (int64_t)n * each < tail) return kTiffBadIfd;
    *n_entries = n;
    const uint8_t *p = f + off + head + (int64_t)n * each;
    *next = o.big ? tiff_u64(p, o.be) : tiff_u32(p, o.be);
    return kTiffOk;
}

// Entry k of the IFD at `off` (which tiff_read_ifd has accepted): kTiffBadValue for a value that does not lie inside the file.
// A type that holds no unsigned number gives at = -1 with kTiffOk: who needs the tag finds it unreadable, nobody else minds.
ZS_HD int tiff_read_entry(const uint8_t *f, int64_t len, TiffOrder o, uint64_t off, uint64_t k, TiffEntry *e) {
    const int64_t head = o.big ? 8 : 2, each = o.big ? 20 : 12, inline_bytes = o.big ? 8 : 4;
    const uint8_t *p = f + off + head + (int64_t)k * each;
    e->tag = (int)tiff_u16(p, o.be), e->type = (int)tiff_u16(p + 2, o.be);
    e->count = o.big ? tiff_u64(p + 4, o.be) : tiff_u32(p + 4, o.be);
    const int64_t value_at = (int64_t)(p - f) + (o.big ? 12 : 8);
    const int size = tiff_type_bytes(e->type);
    e->at = -1;
    if (size == 0 || e->count == 0) return kTiffOk;
    if (e->count > (uint64_t)len) return kTiffBadValue;  // (more values than the file has bytes)
    const int64_t bytes = (int64_t)e->count * size;
    if (bytes <= inline_bytes) {
        e->at = value_at;
        return kTiffOk;
    }
    const uint64_t where = o.big ? tiff_u64(f + value_at, o.be) : tiff_u32(f + value_at, o.be);
    if (where > (uint64_t)len || len - (int64_t)where < bytes) return kTiffBadValue;
    e->at = (int64_t)where;
    return kTiffOk;
}

// The whole walk of page `page`.  kTiffOk and *info; the first `cap` chunks in chunks[] (may be null with cap 0), each with
// status 0 or the library's code for a body that the file ends in.  Otherwise the file's error, with n_pages and the order
// in *info as far as the walk got.
inline int tiff_walk(const uint8_t *f, int64_t len, int64_t page, TiffInfo *info, TiffChunk *chunks, int64_t cap) {
    *info = TiffInfo{};
    TiffOrder o{false, false};
    uint64_t first = 0;
    int rc = tiff_read_header(f, len, &o, &first);
    if (rc != kTiffOk) return rc;
    info->big_endian = o.be, info->bigtiff = o.big;
    // ---- the chain: every IFD once (a second pointer walks at half the speed; where the two meet, the chain loops)
    uint64_t at = first, slow = first, page_off = 0, page_entries = 0;
    int64_t n_pages = 0;
    while (at != 0) {
        uint64_t n = 0, next = 0;
        rc = tiff_read_ifd(f, len, o, at, &n, &next);
        if (rc != kTiffOk) return rc;
        if (n_pages == page) page_off = at, page_entries = n;
        n_pages++;
        at = next;
        if ((n_pages & 1) == 0) {
            uint64_t sn = 0, snext = 0;
            (void)tiff_read_ifd(f, len, o, slow, &sn, &snext);  // (accepted before)
            slow = snext;
        }
        if (at != 0 && at == slow) return kTiffLoop;
    }
    info->n_pages = n_pages;
    if (page < 0 || page >= n_pages) return kTiffNoPage;
    // ---- the page's tags, with the specification's defaults
    uint64_t width = 0, height = 0, bits = 1, spp = 1, compression = 1, predictor = 1, planar = 1, fill_order = 1, sample_format = 1, photometric = 0;
    uint64_t rows_per_strip = 0xFFFFFFFFu, tile_w = 0, tile_h = 0, orientation = 1;
    bool has_w = false, has_h = false, has_tile_w = false, has_tile_h = false, bits_equal = true;
    TiffEntry strip_off{0, 0, 0, -1}, strip_len{0, 0, 0, -1}, tile_off{0, 0, 0, -1}, tile_len{0, 0, 0, -1};
    for (uint64_t k = 0; k < page_entries; k++) {
        TiffEntry e;
        rc = tiff_read_entry(f, len, o, page_off, k, &e);
        const bool ours = e.tag == 256 || e.tag == 257 || e.tag == 258 || e.tag == 259 || e.tag == 262 || e.tag == 266 || e.tag == 273 || e.tag == 274 || e.tag == 277 ||
                          e.tag == 278 || e.tag == 279 || e.tag == 284 || e.tag == 317 || e.tag == 322 || e.tag == 323 || e.tag == 324 || e.tag == 325 || e.tag == 338 ||
                          e.tag == 339;
        if (!ours) continue;  // (what nobody reads may lie anywhere)
        if (rc != kTiffOk) return rc;
        if (e.at < 0) return kTiffBadValue;
        const uint64_t v = tiff_entry_value(f, e, 0, o.be);
        switch (e.tag) {
        case 256: width = v, has_w = true; break;
        case 257: height = v, has_h = true; break;
        case 258:
            bits = v;
            for (uint64_t j = 1; j < e.count; j++) bits_equal = bits_equal && tiff_entry_value(f, e, j, o.be) == v;
            break;
        case 259: compression = v; break;
        case 262: photometric = v; break;
        case 266: fill_order = v; break;
        case 273: strip_off = e; break;
        case 274: orientation = v; break;
        case 277: spp = v; break;
        case 278: rows_per_strip = v; break;
        case 279: strip_len = e; break;
        case 284: planar = v; break;
        case 317: predictor = v; break;
        case 322: tile_w = v, has_tile_w = true; break;
        case 323: tile_h = v, has_tile_h = true; break;
        case 324: tile_off = e; break;
        case 325: tile_len = e; break;
        case 338: info->extra_samples = (int)(e.count > 255 ? 255 : e.count), info->extra_kind = (int)(v & 0xFFFF); break;
        default: sample_format = v; break;  // 339
        }
    }
    if (!has_w || !has_h) return kTiffMissingTag;
    if (width < 1 || height < 1 || width > 0x7FFFFFFFu || height > 0x7FFFFFFFu) return kTiffBadDims;
    info->width = (int64_t)width, info->height = (int64_t)height;
    info->compression = (int)(compression & 0xFFFF), info->predictor = (int)(predictor & 0xFFFF), info->planar = (int)(planar & 0xFFFF);
    info->photometric = (int)(photometric & 0xFFFF), info->sample_format = (int)(sample_format & 0xFFFF), info->orientation = (int)(orientation & 0xFFFF);
    info->bits = (int)(bits & 0xFFFF), info->spp = (int)(spp & 0xFFFF);
    if (compression != 1 && compression != 8 && compression != 32946) return kTiffBadCompression;
    if (spp < 1 || spp > (uint64_t)kTiffMaxSpp) return kTiffBadSamples;
    if (!bits_equal || !(bits == 1 || bits == 2 || bits == 4 || bits == 8 || bits == 16 || bits == 32)) return kTiffBadBits;
    if (predictor < 1 || predictor > 3) return kTiffBadPredictor;
    if (predictor == 2 && bits < 8) return kTiffBadPredictor;
    if (predictor == 3 && (bits != 32 || sample_format != 3)) return kTiffBadPredictor;
    if (planar != 1 && !(planar == 2 && spp == 1)) return kTiffBadPlanar;
    if (fill_order != 1) return kTiffBadFillOrder;
    if (photometric == 6) return kTiffYCbCr;
    const bool tiled = has_tile_w || has_tile_h || tile_off.at >= 0;
    info->tiled = tiled;
    const TiffEntry &offs = tiled ? tile_off : strip_off, &lens = tiled ? tile_len : strip_len;
    if (offs.at < 0 || lens.at < 0) return kTiffMissingTag;
    int64_t across = 1, down;
    if (tiled) {
        if (!has_tile_w || !has_tile_h) return kTiffMissingTag;
        if (tile_w < 16 || tile_h < 16 || tile_w % 16 || tile_h % 16 || tile_w > 0x7FFFFFF0u || tile_h > 0x7FFFFFF0u) return kTiffBadChunkSize;
        info->chunk_w = (int64_t)tile_w, info->chunk_h = (int64_t)tile_h;
        across = tiff_ceil_div(info->width, info->chunk_w), down = tiff_ceil_div(info->height, info->chunk_h);
    } else {
        if (rows_per_strip < 1) return kTiffBadChunkSize;
        info->chunk_w = info->width, info->chunk_h = rows_per_strip > height ? (int64_t)height : (int64_t)rows_per_strip;
        down = tiff_ceil_div(info->height, info->chunk_h);
    }
    info->n_chunks = across * down;  // (below 2^62: both factors are below 2^31)
    if (offs.count != (uint64_t)info->n_chunks || lens.count != (uint64_t)info->n_chunks) return kTiffBadCount;
    info->row_bytes = tiff_row_bytes(info->width, info->spp, info->bits);  // (below 2^31 * 8 * 32 / 8 = 2^36)
    if (info->row_bytes > kTiffMaxLen || info->height > kTiffMaxLen / info->row_bytes) return kTiffTooLarge;
    info->out_len = info->height * info->row_bytes;
    // a chunk's own bytes must be a length too (a tile may be larger than the image)
    const int64_t chunk_row = tiff_row_bytes(info->chunk_w, info->spp, info->bits);
    if (chunk_row > kTiffMaxLen || info->chunk_h > kTiffMaxLen / chunk_row) return kTiffTooLarge;
    for (int64_t i = 0; i < info->n_chunks && i < cap; i++) {
        TiffChunk c{};
        const uint64_t off = tiff_entry_value(f, offs, (uint64_t)i, o.be), n = tiff_entry_value(f, lens, (uint64_t)i, o.be);
        c.x = (i % across) * info->chunk_w, c.y = (i / across) * info->chunk_h;
        c.w = info->width - c.x < info->chunk_w ? info->width - c.x : info->chunk_w;
        c.h = info->height - c.y < info->chunk_h ? info->height - c.y : info->chunk_h;
        const bool inside = off <= (uint64_t)len && n <= (uint64_t)len - off;
        c.off = inside ? (int64_t)off : 0, c.comp_len = inside ? (int64_t)n : 0;
        c.status = inside ? 0 : tiff_err_status(kTiffTruncated);
        chunks[i] = c;
    }
    return kTiffOk;
}

// ---- the writer: a classic little-endian file, [header | IFD | the IFD's longer values | the chunks, each at an even offset]
ZS_HD void tiff_put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8); }
ZS_HD void tiff_put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24); }

// What one image is written as (zs_tiff_put of include/zsgpu.h without its pointer, the defaults resolved)
struct TiffLayout {
    int64_t width, height;
    int bits, spp, sample_format, photometric, extra_samples, extra_kind, predictor;
    int64_t chunk_w, chunk_h;  // a tile, or width x rows per strip
    int tiled;
    int64_t across, n_chunks;
};
// rows per strip where the caller names none: strips of about `kTiffStripBytes` raw bytes (KT, has the
// measurements behind the figure)
constexpr int64_t kTiffStripBytes = 256 << 10;
ZS_HD int64_t tiff_default_rows(int64_t row_bytes, int64_t height) {
    int64_t rows = kTiffStripBytes / (row_bytes > 0 ? row_bytes : 1);
    rows = rows < 1 ? 1 : rows;
    return rows > height ? height : rows;
}
ZS_HD int tiff_n_tags(const TiffLayout &l) { return 12 + (l.tiled ? 1 : 0) + (l.extra_samples > 0 ? 1 : 0); }
// bytes of header, IFD and the values behind it: everything in front of the first chunk (even)
ZS_HD int64_t tiff_head_bytes(const TiffLayout &l) {
    int64_t b = 8 + 2 + 12 * (int64_t)tiff_n_tags(l) + 4;
    if (l.spp > 2) b += 2 * (2 * (int64_t)l.spp);                                  // BitsPerSample, SampleFormat
    if (l.extra_samples > 2) b += 2 * (int64_t)l.extra_samples;
    b = (b + 3) & ~(int64_t)3;
    if (l.n_chunks > 1) b += 2 * 4 * l.n_chunks;  // offsets, byte counts
    return b;
}
// The head of the file into p[0 .. tiff_head_bytes): comp_len[i] is chunk i's length; returns the file's length.  Chunk i
// lies at chunk_off[i] (written here, may be null).
inline int64_t tiff_put_head(uint8_t *p, const TiffLayout &l, const int64_t *comp_len, int64_t *chunk_off) {
    const int64_t head = tiff_head_bytes(l);
    for (int64_t i = 0; i < head; i++) p[i] = 0;
    p[0] = 'I', p[1] = 'I', tiff_put16(p + 2, 42), tiff_put32(p + 4, 8);
    const int n_tags = tiff_n_tags(l);
    tiff_put16(p + 8, (uint32_t)n_tags);
    uint8_t *e = p + 10;
    int64_t extra = 10 + 12 * (int64_t)n_tags + 4;  // where the next longer value goes
    auto entry = [&](int tag, int type, uint32_t count, uint32_t value) {
        tiff_put16(e, (uint32_t)tag), tiff_put16(e + 2, (uint32_t)type), tiff_put32(e + 4, count);
        if (type == 3 && count == 1) tiff_put16(e + 8, value);
        else tiff_put32(e + 8, value);
        e += 12;
    };
    // `count` shorts that all hold `value`
    auto shorts = [&](int tag, uint32_t count, uint32_t value) {
        if (count <= 2) {
            entry(tag, 3, count, count == 2 ? value | value << 16 : value);
        } else {
            entry(tag, 3, count, (uint32_t)extra);
            for (uint32_t k = 0; k < count; k++) tiff_put16(p + extra + 2 * k, value);
            extra += 2 * (int64_t)count;
        }
    };
    // the chunks' places: behind the head, each at an even offset
    int64_t at = head, arrays = 0;
    entry(256, 4, 1, (uint32_t)l.width);
    entry(257, 4, 1, (uint32_t)l.height);
    shorts(258, (uint32_t)l.spp, (uint32_t)l.bits);
    entry(259, 3, 1, 8);
    entry(262, 3, 1, (uint32_t)l.photometric);
    uint8_t *e_off = nullptr, *e_len = nullptr;
    if (!l.tiled) e_off = e, e += 12;  // 273
    entry(277, 3, 1, (uint32_t)l.spp);
    if (!l.tiled) {
        entry(278, 4, 1, (uint32_t)l.chunk_h);
        e_len = e, e += 12;  // 279
    }
    entry(284, 3, 1, 1);
    entry(317, 3, 1, (uint32_t)l.predictor);
    if (l.tiled) {
        entry(322, 4, 1, (uint32_t)l.chunk_w);
        entry(323, 4, 1, (uint32_t)l.chunk_h);
        e_off = e, e += 12;  // 324
        e_len = e, e += 12;  // 325
    }
    if (l.extra_samples > 0) shorts(338, (uint32_t)l.extra_samples, (uint32_t)l.extra_kind);
    shorts(339, (uint32_t)l.spp, (uint32_t)l.sample_format);
    tiff_put32(e, 0);  // no next IFD
    extra = (extra + 3) & ~(int64_t)3;
    arrays = extra;
    uint8_t *save = e;
    e = e_off, entry(l.tiled ? 324 : 273, 4, (uint32_t)l.n_chunks, l.n_chunks > 1 ? (uint32_t)arrays : (uint32_t)head);
    e = e_len, entry(l.tiled ? 325 : 279, 4, (uint32_t)l.n_chunks, l.n_chunks > 1 ? (uint32_t)(arrays + 4 * l.n_chunks) : (uint32_t)comp_len[0]);
    e = save;
    for (int64_t i = 0; i < l.n_chunks; i++) {
        if (l.n_chunks > 1) tiff_put32(p + arrays + 4 * i, (uint32_t)at), tiff_put32(p + arrays + 4 * (l.n_chunks + i), (uint32_t)comp_len[i]);
        if (chunk_off) chunk_off[i] = at;
        at += (comp_len[i] + 1) & ~(int64_t)1;
    }
    return at;
}

// ---- the predictor kernels' per-lane step (KT, zs_tiff.hip; tests/cpp/test_tiff_walk.cpp runs the same code over a model
// of the wave).  A lane holds one 16-byte group of a chunk row: E = 16 / S samples of S bytes, sample j of the group being
// sample s0 + j of the row, whose channel is (s0 + j) mod SPP; p0 = s0 mod SPP is the lane's phase -- zero for every lane where
// SPP divides E, else different from lane to lane.

// the group's four little-endian words as E sample values; `swap`: the samples lie most significant byte first
template <int S>
ZS_HD void tiff_unpack(const uint32_t w[4], uint32_t *v, bool swap) {
    constexpr int E = 16 / S;
#pragma unroll
    for (int j = 0; j < E; j++) {
        if constexpr (S == 1) v[j] = (w[j >> 2] >> (8 * (j & 3))) & 0xFF;
        else if constexpr (S == 2) {
            const uint32_t x = (w[j >> 1] >> (16 * (j & 1))) & 0xFFFF;
            v[j] = swap ? ((x >> 8) | (x << 8)) & 0xFFFF : x;
        } else {
            const uint32_t x = w[j];
            v[j] = swap ? (x >> 24) | ((x >> 8) & 0xFF00) | ((x << 8) & 0xFF0000) | (x << 24) : x;
        }
    }
}
// ... and back, little-endian, each value cut to its S bytes
template <int S>
ZS_HD void tiff_pack(const uint32_t *v, uint32_t w[4]) {
    constexpr int E = 16 / S;
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (int j = 0; j < E; j++) {
        if constexpr (S == 1) w[j >> 2] |= (v[j] & 0xFF) << (8 * (j & 3));
        else if constexpr (S == 2) w[j >> 1] |= (v[j] & 0xFFFF) << (16 * (j & 1));
        else w[j] = v[j];
    }
}
// The sums inside the group: v[j] += v[j - SPP], ascending; tot[c]: the sum of the group's samples of channel c, which is the
// last such sample's value, or 0 where the group has none (SPP > E).
template <int E, int SPP>
ZS_HD void tiff_lane_scan(uint32_t *v, int p0, uint32_t *tot) {
#pragma unroll
    for (int c = 0; c < SPP; c++) tot[c] = 0;
    int ch = p0;
#pragma unroll
    for (int j = 0; j < E; j++) {
        if (j >= SPP) v[j] += v[j - SPP];
#pragma unroll
        for (int c = 0; c < SPP; c++) tot[c] = ch == c ? v[j] : tot[c];
        ch = ch + 1 == SPP ? 0 : ch + 1;
    }
}
// add[c] -- what the row holds of channel c in front of the group -- onto every sample of that channel
template <int E, int SPP>
ZS_HD void tiff_lane_add(uint32_t *v, int p0, const uint32_t *add) {
    int ch = p0;
#pragma unroll
    for (int j = 0; j < E; j++) {
        uint32_t a = 0;
#pragma unroll
        for (int c = 0; c < SPP; c++) a = ch == c ? add[c] : a;
        v[j] += a;
        ch = ch + 1 == SPP ? 0 : ch + 1;
    }
}
// the phase of group g
template <int E, int SPP>
ZS_HD int tiff_phase(int64_t g) {
    if constexpr (E % SPP == 0) return 0;
    else return (int)((g * E) % SPP);
}

// One chunk of a predictor launch, either direction.  `chunk` is the chunk's own bytes, rows of `chunk_pitch` bytes of which
// `nb` are samples (the sums run over all of them); `image` is the chunk's place in the row-major image, rows of `image_pitch`
// bytes, of which `cb` bytes and `rows_in` rows lie inside the image.
struct TiffJob {
    uint8_t *chunk;
    uint8_t *image;
    int64_t chunk_pitch, image_pitch;
    int32_t rows;     // the launch's rows of this chunk: rows_in for the undo, the chunk's full height for the forward kernel
    int32_t rows_in;
    int32_t nb, cb;
    uint8_t sample_bytes;  // 1, 2, 4 (below 8 bits: 1, the bytes are copied)
    uint8_t spp, predictor, swap;
    int32_t pad;
};

}  // namespace zs
