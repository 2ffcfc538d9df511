// zs_png.h -- PNG scanline reconstruction (PNG specification 9.2), the parts that the device kernel (zs_png.hip, KU) and the
// host model (tests/cpp/test_png_unfilter.cpp) share: the per-byte step, the rule that cuts an image into independent
// segments, and the schedule that spreads one segment over the waves of a workgroup.
//
// Schedule.  A segment is a run of rows that reads nothing above its first row.  It is cut into bands of 64 rows; band k
// goes to wave k % W.  Inside a band lane L owns row L and at inner step t reconstructs pixel column t - L (the skewed
// wavefront): its `a` is its own previous result, its `b` is what lane L-1 produced one step earlier and its `c` the `b`
// of the step before.  Time advances in chunk steps of 64 inner steps, the same for all waves, with a barrier between
// them.  In chunk step q of its band a wave takes in tile column q (64 pixel columns of its 64 rows), and because of the
// skew finishes tile column q-1; a band therefore lasts (tile columns + 1) chunk steps.  Band k starts two chunk steps
// after band k-1, so that the row above its lane 0 is complete one tile column ahead of it, and not before band k-W has
// left its wave (png_band_off).
#pragma once

#include <cstdint>

#include "zs_core.h"

namespace zs {

constexpr int kPngRows = 64;     // rows of a band = lanes of a wave
constexpr int kPngChunk = 64;    // pixel columns of a tile column = inner steps of a chunk step
constexpr int kPngRing = 128;    // pixel columns a wave's tile holds: the one being taken in and the one being finished
constexpr int kPngBndBytes = 2 * kPngChunk * 8;  // a wave's incoming boundary row: two tile columns of up to 8-byte pixels

// A row that does not read the prior row starts a segment (None, Sub).  A row with an invalid type byte is reconstructed as
// None (the image is reported; its output is unspecified), so it cuts too.
ZS_HD bool png_row_cuts(int ft) { return ft <= 1 || ft > 4; }

// Which predictor a row's type selects, as masks: the type differs from lane to lane, and a branch per type would run
// every lane through every predictor's code in turn.  All four are computed and one survives the masks.
struct PngSel {
    int a, b, avg, paeth;  // all ones or zero
};
ZS_HD PngSel png_sel(int ft) { return PngSel{-(int)(ft == 1), -(int)(ft == 2), -(int)(ft == 3), -(int)(ft == 4)}; }

ZS_HD int png_paeth_pred(int a, int b, int c) {
    const int pa = b > c ? b - c : c - b, pb = a > c ? a - c : c - a;
    int pc = a + b - 2 * c;
    pc = pc < 0 ? -pc : pc;
    const int bc = pb <= pc ? b : c;
    return ((pa <= pb) & (pa <= pc)) ? a : bc;
}

// Recon(x) = Filt(x) + predictor, mod 256
ZS_HD int png_recon_byte(const PngSel &s, int x, int a, int b, int c) {
    const int pr = (a & s.a) | (b & s.b) | (((a + b) >> 1) & s.avg) | (png_paeth_pred(a, b, c) & s.paeth);
    return (x + pr) & 255;
}

// ... for the BPP bytes of a pixel packed into 64 bits, byte j of the pixel in bits 8j..8j+7
template <int BPP>
ZS_HD uint64_t png_recon_px(const PngSel &s, uint64_t x, uint64_t a, uint64_t b, uint64_t c) {
    uint64_t r = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < BPP; j++)
        r |= (uint64_t)png_recon_byte(s, (int)(x >> (8 * j)) & 255, (int)(a >> (8 * j)) & 255, (int)(b >> (8 * j)) & 255,
                                      (int)(c >> (8 * j)) & 255)
             << (8 * j);
    return r;
}

ZS_HD int64_t png_npx(int64_t row_bytes, int bpp) { return (row_bytes + bpp - 1) / bpp; }  // (the last pixel may be partial)
ZS_HD int64_t png_nq(int64_t npx) { return (npx + kPngChunk - 1) / kPngChunk + 1; }        // chunk steps of a band
// a wave takes its next band `period` chunk steps after the last one: after that band's end, and so that the start of
// band k stays two chunk steps behind band k-1 where the bands wrap around the waves
ZS_HD int64_t png_period(int64_t nq, int waves) { return nq + 1 > 2 * (int64_t)waves ? nq + 1 : 2 * (int64_t)waves; }
ZS_HD int64_t png_band_off(int64_t k, int waves, int64_t nq) { return 2 * (k % waves) + (k / waves) * png_period(nq, waves); }
ZS_HD int64_t png_total_steps(int64_t nbands, int waves, int64_t nq) { return png_band_off(nbands - 1, waves, nq) + nq; }

// bytes between two rows of a wave's tile: kPngRing pixels and a pad that puts lane L's pixel of one inner step
// (row L, column t - L) on bank L
ZS_HD constexpr int png_tile_stride(int bpp) { return kPngRing * bpp + ((bpp + 3) & ~3) + (bpp > 4 ? 8 : 4); }
ZS_HD constexpr int png_lds_bytes(int max_bpp, int waves) { return waves * (kPngRows * png_tile_stride(max_bpp) + kPngBndBytes); }
// four waves per workgroup while a pixel has at most 4 bytes, two above that: either way the largest tiles take ~134 KiB
// of a CU's 160 KiB
ZS_HD constexpr int png_waves(int max_bpp) { return max_bpp <= 4 ? 4 : 2; }

// ---- filtering a batch (zs_png_filter_batch_kernel, KP) ----
// The grid is the flat list of all images' rows.  row_off[i] = rows of the images before i, row_off[n] = all rows; every
// image has at least one row, so the offsets increase strictly.  The image of flat row r is the last i with
// row_off[i] <= r (the same for every thread of a workgroup: a uniform search, no divergence).
template <class Off>
ZS_HD int png_row_image(const Off &row_off, int n, int64_t r) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)row_off[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- Adam7 (PNG specification 8.2): the pass geometry, and the gather that KA (zs_png.hip) and its host model
// (tests/cpp/test_png_adam7.cpp) share ----
// Pass p = 0..6 (the specification's 1..7) holds the pixels (xstart + k * xstep, ystart + j * ystep); the steps are powers
// of two, kept as shifts.  One nibble per pass, pass 0 in the lowest.
constexpr int kAdam7Passes = 7;
ZS_HD int adam7_xstart(int p) { return (0x0102040 >> (4 * p)) & 15; }  // 0 4 0 2 0 1 0
ZS_HD int adam7_ystart(int p) { return (0x1020400 >> (4 * p)) & 15; }  // 0 0 4 0 2 0 1
ZS_HD int adam7_xshift(int p) { return (0x0112233 >> (4 * p)) & 15; }  // steps 8 8 4 4 2 2 1
ZS_HD int adam7_yshift(int p) { return (0x1122333 >> (4 * p)) & 15; }  // steps 8 8 8 4 4 2 2
ZS_HD int64_t adam7_span(int64_t n, int start, int shift) { return n > start ? (n - start + ((int64_t)1 << shift) - 1) >> shift : 0; }
ZS_HD int64_t adam7_pass_width(int64_t w, int p) { return adam7_span(w, adam7_xstart(p), adam7_xshift(p)); }
ZS_HD int64_t adam7_pass_height(int64_t h, int p) { return adam7_span(h, adam7_ystart(p), adam7_yshift(p)); }

ZS_HD bool png_bits_ok(int bits) { return bits == 1 || bits == 2 || bits == 4 || (bits >= 8 && bits <= 64 && bits % 8 == 0 && bits != 40 && bits != 56); }
ZS_HD int64_t png_bits_row_bytes(int64_t w, int bits) { return (w * bits + 7) >> 3; }
ZS_HD int png_bits_bpp(int bits) { return bits < 8 ? 1 : bits >> 3; }  // what the filters call bpp

// The inverse map: the pass of output pixel (x, y) and its place inside that pass.  Per output row the sources are few:
// y % 8 == 0 draws on passes 0, 1, 3 and 5; y % 8 == 4 on 2, 3 and 5; y % 4 == 2 on 4 and 5; odd y on pass 6 alone.
struct Adam7Src {
    int pass;
    int64_t col, row;
};
ZS_HD Adam7Src adam7_source(int64_t x, int64_t y) {
    int p;
    if (y & 1) p = 6;
    else if (x & 1) p = 5;
    else if (y & 2) p = 4;
    else if (x & 2) p = 3;
    else if (y & 4) p = 2;
    else if (x & 4) p = 1;
    else p = 0;
    return Adam7Src{p, x >> adam7_xshift(p), y >> adam7_yshift(p)};  // (the start is below the step: the shift drops it)
}

// One interlaced image for KA.  passes: the reconstructed passes back to back (no filter bytes, absent passes absent);
// off[p]: where pass p starts in it; out: height rows of png_bits_row_bytes(width, bits) bytes.
struct Adam7Img {
    const uint8_t *passes;
    uint8_t *out;
    int64_t off[kAdam7Passes];
    int32_t width, height, bits, pad;
};
// ... filled in from the geometry; returns the bytes of all passes
ZS_HD int64_t adam7_layout(Adam7Img &im) {
    int64_t at = 0;
    for (int p = 0; p < kAdam7Passes; p++) {
        im.off[p] = at;
        at += png_bits_row_bytes(adam7_pass_width(im.width, p), im.bits) * adam7_pass_height(im.height, p);
    }
    return at;
}

constexpr int kAdam7GroupBits = 4;  // output bytes a thread builds at 1, 2 and 4 bits a pixel (8 .. 32 pixels)

ZS_HD const uint8_t *adam7_pass_row(const Adam7Img &im, int p, int64_t row) {
    return im.passes + im.off[p] + row * png_bits_row_bytes(adam7_pass_width(im.width, p), im.bits);
}

// Output byte b of row y at 1, 2 or 4 bits a pixel: the 8 / 4 / 2 pixels that land in it, leftmost in the high bits, each
// from its own pass row; pixels past the width leave zero bits.
ZS_HD uint32_t adam7_bits_byte(const Adam7Img &im, int64_t y, int64_t b) {
    const int bits = im.bits, ppb = 8 / bits;
    uint32_t v = 0;
    for (int j = 0; j < ppb; j++) {
        const int64_t x = b * ppb + j;
        if (x >= im.width) break;
        const Adam7Src s = adam7_source(x, y);
        const int64_t bit = s.col * bits;
        const uint32_t byte = adam7_pass_row(im, s.pass, s.row)[bit >> 3];
        v |= ((byte >> (8 - bits - (int)(bit & 7))) & ((1u << bits) - 1)) << (8 - bits - j * bits);
    }
    return v;
}

// Bytes [b0, b0 + G) of output row y (`dst` = the row's first byte, `rb` its length; dst + b0 is G-aligned, so the first
// group of a row may begin in front of it and the last one end behind it: those two store byte by byte, every other group
// is one aligned store of G bytes).  G = 4, 8 or 16.  No byte outside [0, rb) is touched, and none is touched twice.
template <int G>
ZS_HD void adam7_group(const Adam7Img &im, int64_t y, int64_t rb, uint8_t *dst, int64_t b0) {
    static_assert(G == 4 || G == 8 || G == 16, "a group is one store");
    uint64_t v[2] = {0, 0};  // byte k of the group in bits 8k.. of v[k / 8]
    const int64_t lo = b0 < 0 ? 0 : b0, hi = b0 + G < rb ? b0 + G : rb;  // the group's bytes inside the row
    const bool full = lo == b0 && hi == b0 + G;
    if (y & 1) {
        // an odd row is pass 6's row as it stands (its columns are the image's)
        const uint8_t *src = adam7_pass_row(im, 6, y >> 1);
        if (full) __builtin_memcpy(v, src + b0, G);
        else
            for (int64_t b = lo; b < hi; b++) v[(b - b0) >> 3] |= (uint64_t)src[b] << (8 * ((b - b0) & 7));
        const int used = (int)(((int64_t)im.width * im.bits) & 7);  // bits of the row's last byte that hold pixels (0: all)
        if (used && hi == rb) {
            const int k = (int)(rb - 1 - b0);
            v[k >> 3] &= ~((uint64_t)(0xFFu >> used) << (8 * (k & 7)));
        }
    } else if (im.bits < 8) {
        for (int64_t b = lo; b < hi; b++) v[(b - b0) >> 3] |= (uint64_t)adam7_bits_byte(im, y, b) << (8 * ((b - b0) & 7));
    } else {
        // whole pixels of bpp bytes; the first and the last may lie partly in a neighbouring group
        const int bpp = im.bits >> 3;
        for (int64_t x = lo / bpp; x * bpp < hi; x++) {
            const Adam7Src s = adam7_source(x, y);
            const uint8_t *src = adam7_pass_row(im, s.pass, s.row) + s.col * bpp;
            uint64_t px = 0;
            switch (bpp) {
            case 1: px = src[0]; break;
            case 2: __builtin_memcpy(&px, src, 2); break;
            case 3: __builtin_memcpy(&px, src, 3); break;
            case 4: __builtin_memcpy(&px, src, 4); break;
            case 6: __builtin_memcpy(&px, src, 6); break;
            default: __builtin_memcpy(&px, src, 8); break;
            }
            int o = (int)(x * bpp - b0);  // the pixel's first byte in the group: -7 .. G - 1
            if (o < 0) px >>= -8 * o, o = 0;
            if (o < 8) {
                v[0] |= px << (8 * o);
                if (o > 0) v[1] |= px >> (8 * (8 - o));
            } else
                v[1] |= px << (8 * (o - 8));
        }
        // (bytes of the last pixel behind the group fell off v[1], or sit in it above byte G and are not stored)
    }
    if (full) {
        __builtin_memcpy(__builtin_assume_aligned(dst + b0, G), v, G);
    } else
        for (int64_t b = lo; b < hi; b++) dst[b] = (uint8_t)(v[(b - b0) >> 3] >> (8 * ((b - b0) & 7)));
}

// groups of G bytes that cover a row of rb bytes beginning at address `row_addr`, and the first one's b0 (<= 0)
ZS_HD int64_t adam7_row_groups(uint64_t row_addr, int64_t rb, int G) { return ((int64_t)(row_addr & (uint64_t)(G - 1)) + rb + G - 1) / G; }
ZS_HD int64_t adam7_row_b0(uint64_t row_addr, int G) { return -(int64_t)(row_addr & (uint64_t)(G - 1)); }

// ---- the Adam7 split (KS, zs_png.hip, and its host model tests/cpp/test_png_adam7_split.cpp): KA's inverse ----
// One image for KS.  pixels: height rows of png_bits_row_bytes(width, bits) bytes; passes: where the present passes go, back
// to back (adam7_layout's picture: off[p]); row0[p]: pass rows of the image in front of pass p, row0[7] all of them -- the
// image's share of the flat list of pass rows.  An absent pass has no rows.
struct Adam7SplitImg {
    const uint8_t *pixels;
    uint8_t *passes;
    int64_t off[kAdam7Passes];
    int32_t row0[kAdam7Passes + 1];
    int32_t width, height, bits, pad;
};
// ... filled in from the geometry; returns the bytes of all passes (row0[7]: the pass rows, below 2^31 for every legal image:
// at most 15 for every 8 of its own, and the callers bound the sum)
ZS_HD int64_t adam7_split_layout(Adam7SplitImg &im) {
    int64_t at = 0, rows = 0;
    for (int p = 0; p < kAdam7Passes; p++) {
        const int64_t pw = adam7_pass_width(im.width, p), ph = adam7_pass_height(im.height, p);
        im.off[p] = at;
        im.row0[p] = (int32_t)rows;
        at += png_bits_row_bytes(pw, im.bits) * ph;
        rows += pw > 0 ? ph : 0;
    }
    im.row0[kAdam7Passes] = (int32_t)rows;
    return at;
}
ZS_HD int64_t adam7_pass_rows(int64_t w, int64_t h) {  // pass rows of an interlaced image, absent passes left out
    int64_t rows = 0;
    for (int p = 0; p < kAdam7Passes; p++) rows += adam7_pass_width(w, p) > 0 ? adam7_pass_height(h, p) : 0;
    return rows;
}
// the pass of the image's pass row r (0 <= r < row0[7]): the last present one that begins at or in front of it
ZS_HD int adam7_split_pass(const Adam7SplitImg &im, int64_t r) {
    int p = 0;
    for (int q = 1; q < kAdam7Passes; q++)
        if (im.row0[q + 1] > im.row0[q] && r >= im.row0[q]) p = q;
    return p;
}

ZS_HD uint64_t adam7_load_px(const uint8_t *src, int bpp) {  // a pixel of 1, 2, 3, 4, 6 or 8 bytes at any alignment
    uint64_t px = 0;
    switch (bpp) {
    case 1: px = src[0]; break;
    case 2: __builtin_memcpy(&px, src, 2); break;
    case 3: __builtin_memcpy(&px, src, 3); break;
    case 4: __builtin_memcpy(&px, src, 4); break;
    case 6: __builtin_memcpy(&px, src, 6); break;
    default: __builtin_memcpy(&px, src, 8); break;
    }
    return px;
}

// Bytes [b0, b0 + G) of row j of pass p (`dst` = the pass row's first byte, `prb` its length; dst + b0 is G-aligned: the
// first group of a row may begin in front of it and the last one end behind it, those two store byte by byte, every other
// group is one aligned store of G bytes).  G = 4, 8 or 16.  Output pixel k is source pixel xstart + (k << xshift) of source
// row ystart + (j << yshift).  No byte outside [0, prb) is touched, and none is touched twice; the unused low bits of the
// pass row's last byte are zero, and the unused bits of the source row's last byte are never taken over.
template <int G>
ZS_HD void adam7_split_group(const Adam7SplitImg &im, int p, int64_t j, int64_t prb, uint8_t *dst, int64_t b0) {
    static_assert(G == 4 || G == 8 || G == 16, "a group is one store");
    uint64_t v[2] = {0, 0};  // byte k of the group in bits 8k.. of v[k / 8]
    const int64_t lo = b0 < 0 ? 0 : b0, hi = b0 + G < prb ? b0 + G : prb;  // the group's bytes inside the row
    const bool full = lo == b0 && hi == b0 + G;
    const int xs = adam7_xstart(p), xsh = adam7_xshift(p), bits = im.bits;
    const uint8_t *src = im.pixels + (adam7_ystart(p) + (j << adam7_yshift(p))) * png_bits_row_bytes(im.width, bits);
    if (xsh == 0) {
        // pass 7's rows are the odd source rows as they stand
        if (full) __builtin_memcpy(v, src + b0, G);
        else
            for (int64_t b = lo; b < hi; b++) v[(b - b0) >> 3] |= (uint64_t)src[b] << (8 * ((b - b0) & 7));
        const int used = (int)(((int64_t)im.width * bits) & 7);  // bits of the row's last byte that hold pixels (0: all)
        if (used && hi == prb) {
            const int k = (int)(prb - 1 - b0);
            v[k >> 3] &= ~((uint64_t)(0xFFu >> used) << (8 * (k & 7)));
        }
    } else if (bits < 8) {
        // an output byte collects 8 / 4 / 2 pixels of the one source row, leftmost in the high bits
        const int ppb = 8 / bits;
        const int64_t pw = adam7_pass_width(im.width, p);
        for (int64_t b = lo; b < hi; b++) {
            uint32_t byte = 0;
            for (int q = 0; q < ppb; q++) {
                const int64_t k = b * ppb + q;
                if (k >= pw) break;
                const int64_t bit = (xs + (k << xsh)) * bits;
                byte |= (((uint32_t)src[bit >> 3] >> (8 - bits - (int)(bit & 7))) & ((1u << bits) - 1)) << (8 - bits - q * bits);
            }
            v[(b - b0) >> 3] |= (uint64_t)byte << (8 * ((b - b0) & 7));
        }
    } else {
        // whole pixels of bpp bytes; the first and the last may lie partly in a neighbouring group
        const int bpp = bits >> 3;
        for (int64_t k = lo / bpp; k * bpp < hi; k++) {
            uint64_t px = adam7_load_px(src + (xs + (k << xsh)) * bpp, bpp);
            int o = (int)(k * bpp - b0);  // the pixel's first byte in the group: -7 .. G - 1
            if (o < 0) px >>= -8 * o, o = 0;
            if (o < 8) {
                v[0] |= px << (8 * o);
                if (o > 0) v[1] |= px >> (8 * (8 - o));
            } else
                v[1] |= px << (8 * (o - 8));
        }
    }
    if (full) {
        __builtin_memcpy(__builtin_assume_aligned(dst + b0, G), v, G);
    } else
        for (int64_t b = lo; b < hi; b++) dst[b] = (uint8_t)(v[(b - b0) >> 3] >> (8 * ((b - b0) & 7)));
}

// ---- expansion to RGBA (KX, zs_png.hip, and its host model tests/cpp/test_png_expand.cpp) ----
// Raw scanlines of any legal (colour type, bit depth) pair -> rows of width * 4 bytes (R, G, B, A) or of width * 4 uint16 in
// host order (R, G, B, A), no padding.  Exact integer arithmetic:
//   a sample v of depth d to 8 bits:  d < 8: v * 255 / (2^d - 1) (x255, x85, x17);  d = 8: v;  d = 16: (v * 255 + 32895) >> 16
//   ... to 16 bits:                   d < 16: v * 65535 / (2^d - 1) (x65535, x21845, x4369, x257);  d = 16: v, read big-endian
//   gray (types 0, 4): R = G = B = the scaled sample
//   alpha: types 4, 6: the scaled alpha sample; types 0, 2 with a tRNS key: 0 where the pixel's samples at their original
//          depth equal the key's low d bits (gray: one sample, RGB: all three), the maximum elsewhere; without a key: the maximum
//   palette (type 3): index k -> entry k of the image's 256-entry RGBA8 table, which the host fills from PLTE and tRNS
//          (entries past PLTE: 0, 0, 0, 255), so no index is range-checked; to 16 bits every channel x257
constexpr int ZS_PNG_FMT_RGBA8 = 0, ZS_PNG_FMT_RGBA16 = 1;
ZS_HD constexpr int png_expand_bytes(int format) { return format == ZS_PNG_FMT_RGBA16 ? 8 : 4; }
constexpr int kPngPalEntries = 256;  // a palette image's table: entry k = R | G << 8 | B << 16 | A << 24
constexpr int kPngExpandGroup = 16;  // output bytes of one store: 4 pixels of RGBA8, 2 of RGBA16

struct PngExpandImg {
    const uint8_t *in;  // height rows of ceil(width * depth * channels / 8) bytes
    uint8_t *out;       // height rows of width * png_expand_bytes(format) bytes, aligned to a pixel
    int32_t width, height, depth, color, format;
    int32_t pal_off;    // type 3: the table's first entry in the call's list of tables
    uint16_t key[3];    // tRNS of types 0 (key[0]) and 2: the 16-bit values as the chunk holds them
    uint16_t has_key;
};

// the host's share: the table of a palette image from its PLTE (entries * 3 bytes) and tRNS (trns_len bytes) data
inline void png_expand_table(const uint8_t *plte, int entries, const uint8_t *trns, int trns_len, uint32_t *table) {
    for (int k = 0; k < kPngPalEntries; k++) {
        if (k >= entries) table[k] = 0xFF000000u;
        else table[k] = (uint32_t)plte[3 * k] | (uint32_t)plte[3 * k + 1] << 8 | (uint32_t)plte[3 * k + 2] << 16 | (uint32_t)(k < trns_len ? trns[k] : 255) << 24;
    }
}

template <int F, int D>
ZS_HD uint32_t png_expand_scale(uint32_t v) {
    if constexpr (F == ZS_PNG_FMT_RGBA8) return D == 16 ? (v * 255 + 32895) >> 16 : v * (255u / ((1u << (D < 8 ? D : 8)) - 1));
    else return v * (65535u / ((1u << D) - 1));
}
template <int F>
ZS_HD uint64_t png_expand_pack(uint32_t r, uint32_t g, uint32_t b, uint32_t a) {
    if constexpr (F == ZS_PNG_FMT_RGBA8) return (uint64_t)(r | g << 8 | b << 16 | a << 24);
    else return (uint64_t)r | (uint64_t)g << 16 | (uint64_t)b << 32 | (uint64_t)a << 48;
}

// One pixel from its samples s[0 .. channels) at their original depth (a palette image: s[0] is the index).
template <int F, int CT, int D>
ZS_HD uint64_t png_expand_samples(const PngExpandImg &im, const uint32_t *pal, const uint32_t *s) {
    constexpr uint32_t top = F == ZS_PNG_FMT_RGBA8 ? 255u : 65535u, mask = (1u << D) - 1;
    if constexpr (CT == 3) {
        const uint32_t e = pal[s[0]];
        if constexpr (F == ZS_PNG_FMT_RGBA8) return e;
        else return ((uint64_t)(e & 255) | (uint64_t)(e >> 8 & 255) << 16 | (uint64_t)(e >> 16 & 255) << 32 | (uint64_t)(e >> 24) << 48) * 257;
    } else if constexpr (CT == 0) {
        const uint32_t v = png_expand_scale<F, D>(s[0]);
        return png_expand_pack<F>(v, v, v, im.has_key && s[0] == (im.key[0] & mask) ? 0 : top);
    } else if constexpr (CT == 4) {
        const uint32_t v = png_expand_scale<F, D>(s[0]);
        return png_expand_pack<F>(v, v, v, png_expand_scale<F, D>(s[1]));
    } else if constexpr (CT == 2) {
        const bool keyed = im.has_key && s[0] == (im.key[0] & mask) && s[1] == (im.key[1] & mask) && s[2] == (im.key[2] & mask);
        return png_expand_pack<F>(png_expand_scale<F, D>(s[0]), png_expand_scale<F, D>(s[1]), png_expand_scale<F, D>(s[2]), keyed ? 0 : top);
    } else
        return png_expand_pack<F>(png_expand_scale<F, D>(s[0]), png_expand_scale<F, D>(s[1]), png_expand_scale<F, D>(s[2]), png_expand_scale<F, D>(s[3]));
}

// NPX pixels from x on (all inside the row), pixel j in px[j].  At 8 and 16 bits the bytes that hold them are taken in with
// one copy of constant length; below that a pixel is a part of one byte, and neighbours share bytes.
template <int F, int CT, int D, int NPX>
ZS_HD void png_expand_pixels(const PngExpandImg &im, const uint32_t *pal, const uint8_t *row, int64_t x, uint64_t *px) {
    constexpr int CH = CT == 2 ? 3 : CT == 4 ? 2 : CT == 6 ? 4 : 1;
    if constexpr (D < 8) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < NPX; j++) {
            const int64_t bit = (x + j) * D;
            const uint32_t s = ((uint32_t)row[bit >> 3] >> (8 - D - (int)(bit & 7))) & ((1u << D) - 1);
            px[j] = png_expand_samples<F, CT, D>(im, pal, &s);
        }
    } else {
        constexpr int SB = D / 8, BPP = CH * SB;
        uint8_t raw[NPX * BPP];
        __builtin_memcpy(raw, row + x * BPP, NPX * BPP);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < NPX; j++) {
            uint32_t s[CH];
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < CH; k++) s[k] = SB == 1 ? raw[j * BPP + k] : (uint32_t)raw[j * BPP + 2 * k] << 8 | raw[j * BPP + 2 * k + 1];
            px[j] = png_expand_samples<F, CT, D>(im, pal, s);
        }
    }
}

template <int F, int CT, int D>
ZS_HD void png_expand_group_as(const PngExpandImg &im, const uint32_t *pal, int64_t y, uint8_t *dst, int64_t b0) {
    constexpr int P = png_expand_bytes(F), N = kPngExpandGroup / P;
    constexpr int CH = CT == 2 ? 3 : CT == 4 ? 2 : CT == 6 ? 4 : 1;
    const int64_t rb = (int64_t)im.width * P;
    const int64_t lo = b0 < 0 ? 0 : b0, hi = b0 + kPngExpandGroup < rb ? b0 + kPngExpandGroup : rb;  // the group's bytes inside the row
    const uint8_t *row = im.in + y * png_bits_row_bytes(im.width, D * CH);
    if (lo == b0 && hi == b0 + kPngExpandGroup) {
        uint64_t px[N], v[2];
        png_expand_pixels<F, CT, D, N>(im, pal, row, b0 / P, px);
        if constexpr (F == ZS_PNG_FMT_RGBA8) v[0] = px[0] | px[1] << 32, v[1] = px[2] | px[3] << 32;
        else v[0] = px[0], v[1] = px[1];
        __builtin_memcpy(__builtin_assume_aligned(dst + b0, kPngExpandGroup), v, kPngExpandGroup);
    } else
        for (int64_t b = lo; b < hi; b += P) {  // (dst and b0 are multiples of P: whole pixels)
            uint64_t px;
            png_expand_pixels<F, CT, D, 1>(im, pal, row, b / P, &px);
            __builtin_memcpy(__builtin_assume_aligned(dst + b, P), &px, P);
        }
}

// Bytes [b0, b0 + 16) of output row y (`dst` = the row's first byte, aligned to a pixel; dst + b0 is 16-aligned, so the
// first group of a row may begin in front of it and the last one end behind it: those two store pixel by pixel, every other
// group is one aligned store of 16 bytes).  pal: the image's table (type 3 only).  No byte outside the row is touched,
// and none is touched twice.  The (colour type, depth) pair is the same for a whole row: one jump, then straight code.
template <int F>
ZS_HD void png_expand_group(const PngExpandImg &im, const uint32_t *pal, int64_t y, uint8_t *dst, int64_t b0) {
    switch (im.color * 32 + im.depth) {
    case 0 * 32 + 1: png_expand_group_as<F, 0, 1>(im, pal, y, dst, b0); break;
    case 0 * 32 + 2: png_expand_group_as<F, 0, 2>(im, pal, y, dst, b0); break;
    case 0 * 32 + 4: png_expand_group_as<F, 0, 4>(im, pal, y, dst, b0); break;
    case 0 * 32 + 8: png_expand_group_as<F, 0, 8>(im, pal, y, dst, b0); break;
    case 0 * 32 + 16: png_expand_group_as<F, 0, 16>(im, pal, y, dst, b0); break;
    case 2 * 32 + 8: png_expand_group_as<F, 2, 8>(im, pal, y, dst, b0); break;
    case 2 * 32 + 16: png_expand_group_as<F, 2, 16>(im, pal, y, dst, b0); break;
    case 3 * 32 + 1: png_expand_group_as<F, 3, 1>(im, pal, y, dst, b0); break;
    case 3 * 32 + 2: png_expand_group_as<F, 3, 2>(im, pal, y, dst, b0); break;
    case 3 * 32 + 4: png_expand_group_as<F, 3, 4>(im, pal, y, dst, b0); break;
    case 3 * 32 + 8: png_expand_group_as<F, 3, 8>(im, pal, y, dst, b0); break;
    case 4 * 32 + 8: png_expand_group_as<F, 4, 8>(im, pal, y, dst, b0); break;
    case 4 * 32 + 16: png_expand_group_as<F, 4, 16>(im, pal, y, dst, b0); break;
    case 6 * 32 + 8: png_expand_group_as<F, 6, 8>(im, pal, y, dst, b0); break;
    case 6 * 32 + 16: png_expand_group_as<F, 6, 16>(im, pal, y, dst, b0); break;
    default: break;  // (the host admits the fifteen pairs of table 11.1 only)
    }
}

// ---- packing RGBA into raw scanlines (KG, zs_png.hip, and its host model tests/cpp/test_png_pack.cpp): KX's inverse ----
// Rows of width * 4 bytes (R, G, B, A) or of width * 4 uint16 in host order -> raw scanlines of the (colour type, bit depth)
// pair the caller names, rows of ceil(width * bits / 8) bytes.  Exact integer arithmetic:
//   a sample v to depth d, from RGBA8:   d <= 8: v >> (8 - d);  d = 16: v * 257
//   ...                    from RGBA16:  d = 16: v;  d <= 8: v8 = (v * 255 + 32895) >> 16 (KX's own rounding), then v8 >> (8 - d)
//       (both invert KX's scaling on every value KX can produce)
//   16-bit samples are written big-endian; below 8 bits pixels are packed most-significant-bit first, and the unused low
//   bits of a row's last byte are zero
//   gray (types 0, 4): the R sample; alpha (types 4, 6): the A sample; types 0 and 2 without a tRNS key ignore alpha
//   types 0 and 2 with a key: a pixel whose alpha is 0 gets the key's low d bits in every sample, every other pixel its own
//   palette (type 3): the pixel reduced to RGBA8 by the rule above (d = 8), then the index of the first palette entry equal to
//       it in all four channels (an entry's alpha: trns[k] for k < trns_len, else 255); no equal entry: index 0, and counted
// The palette lookup is a hash table the host builds per image: kPngPackColors words of entries (R | G << 8 | B << 16 |
// A << 24, as KX's table, zero past the PLTE's entries) and behind them kPngPackSlots 16-bit slots, two a word, that hold
// entry index + 1 or 0 for "empty" -- 0x00000000 is a legal colour, so emptiness is not a colour value.  Open addressing,
// linear probing; at most 256 of the 512 slots are taken, so every probe sequence ends.
constexpr int kPngPackColors = 256, kPngPackSlots = 512;
constexpr int kPngPackTableWords = kPngPackColors + kPngPackSlots / 2;  // 2 KiB an image
ZS_HD uint32_t png_color_hash(uint32_t rgba, int bits) { return (rgba * 0x9E3779B1u) >> (32 - bits); }
ZS_HD uint32_t png_pack_slot(const uint32_t *table, uint32_t h) { return (table[kPngPackColors + (h >> 1)] >> (16 * (h & 1))) & 0xFFFFu; }

// the host's share: the table of a palette image.  The first entry wins among duplicates.
inline void png_pack_table(const uint8_t *plte, int entries, const uint8_t *trns, int trns_len, uint32_t *table) {
    for (int k = 0; k < kPngPackTableWords; k++) table[k] = 0;
    for (int k = 0; k < entries; k++) {
        const uint32_t c = (uint32_t)plte[3 * k] | (uint32_t)plte[3 * k + 1] << 8 | (uint32_t)plte[3 * k + 2] << 16 | (uint32_t)(k < trns_len ? trns[k] : 255) << 24;
        table[k] = c;
        uint32_t h = png_color_hash(c, 9);
        for (;;) {
            const uint32_t s = png_pack_slot(table, h);
            if (s == 0) {
                table[kPngPackColors + (h >> 1)] |= (uint32_t)(k + 1) << (16 * (h & 1));
                break;
            }
            if (table[s - 1] == c) break;  // (an earlier entry of the same colour)
            h = (h + 1) & (kPngPackSlots - 1);
        }
    }
}
// the index of colour c, or -1
ZS_HD int png_pack_lookup(const uint32_t *table, uint32_t c) {
    uint32_t h = png_color_hash(c, 9);
    for (int t = 0; t < kPngPackSlots; t++) {  // (an empty slot is met long before)
        const uint32_t s = png_pack_slot(table, h);
        if (s == 0) return -1;
        if (table[s - 1] == c) return (int)s - 1;
        h = (h + 1) & (kPngPackSlots - 1);
    }
    return -1;
}

struct PngPackImg {
    const uint8_t *in;  // height rows of width * png_expand_bytes(format) bytes, aligned to a pixel
    uint8_t *out;       // height rows of ceil(width * depth * channels / 8) bytes, any alignment
    int32_t width, height, depth, color, format;
    int32_t pal_off;    // type 3: the table's first word in the call's list of tables
    uint16_t key[3];    // tRNS of types 0 (key[0]) and 2: the 16-bit values as the chunk holds them
    uint16_t has_key;
};

constexpr int kPngPackGroup = 16;  // output bytes of one store at 8 bits a pixel and above; below: kAdam7GroupBits

template <int F, int D>
ZS_HD uint32_t png_pack_scale(uint32_t v) {
    if constexpr (F == ZS_PNG_FMT_RGBA8) return D == 16 ? v * 257 : v >> (8 - (D < 8 ? D : 8));
    else return D == 16 ? v : ((v * 255 + 32895) >> 16) >> (8 - (D < 8 ? D : 8));
}

// Pixel x of a source row -> its bytes in the file's layout, byte j in bits 8j.. (below 8 bits: the one sample); *miss is
// advanced for a palette pixel without an entry.
template <int F, int CT, int D>
ZS_HD uint64_t png_pack_pixel(const PngPackImg &im, const uint32_t *table, const uint8_t *src, int64_t x, uint32_t *miss) {
    uint32_t c[4];
    if constexpr (F == ZS_PNG_FMT_RGBA8) {
        uint32_t v;
        __builtin_memcpy(&v, __builtin_assume_aligned(src + x * 4, 4), 4);
        c[0] = v & 255, c[1] = v >> 8 & 255, c[2] = v >> 16 & 255, c[3] = v >> 24;
    } else {
        uint64_t v;
        __builtin_memcpy(&v, __builtin_assume_aligned(src + x * 8, 8), 8);
        c[0] = (uint32_t)v & 0xFFFFu, c[1] = (uint32_t)(v >> 16) & 0xFFFFu, c[2] = (uint32_t)(v >> 32) & 0xFFFFu, c[3] = (uint32_t)(v >> 48);
    }
    if constexpr (CT == 3) {
        const uint32_t rgba = png_pack_scale<F, 8>(c[0]) | png_pack_scale<F, 8>(c[1]) << 8 | png_pack_scale<F, 8>(c[2]) << 16 | png_pack_scale<F, 8>(c[3]) << 24;
        const int k = png_pack_lookup(table, rgba);
        if (k < 0) ++*miss;
        return k < 0 ? 0 : (uint64_t)k;
    } else {
        constexpr int CH = CT == 2 ? 3 : CT == 4 ? 2 : CT == 6 ? 4 : 1;
        constexpr uint32_t mask = (1u << D) - 1;
        uint32_t s[CH];
        if constexpr (CT == 0 || CT == 2) {
            const bool keyed = im.has_key && c[3] == 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < CH; k++) s[k] = keyed ? (im.key[k] & mask) : png_pack_scale<F, D>(c[k]);
        } else if constexpr (CT == 4) {
            s[0] = png_pack_scale<F, D>(c[0]), s[1] = png_pack_scale<F, D>(c[3]);
        } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < 4; k++) s[k] = png_pack_scale<F, D>(c[k]);
        }
        uint64_t px = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < CH; k++) {
            if constexpr (D == 16) px |= (uint64_t)((s[k] >> 8) | (s[k] & 255) << 8) << (16 * k);  // big-endian
            else px |= (uint64_t)s[k] << (8 * k);
        }
        return px;
    }
}

// Bytes [b0, b0 + G) of output row y (`dst` = the row's first byte, `rb` its length; dst + b0 is G-aligned, so the first
// group of a row may begin in front of it and the last one end behind it: those two store byte by byte, every other group is
// one aligned store of G bytes).  G = 4, 8 or 16.  No byte outside [0, rb) is touched, and none is touched twice.  Returns
// the palette pixels of the group that found no entry: below 8 bits a pixel lies in one byte, at 8 bits it is one, so each is
// counted by one group.
template <int F, int CT, int D, int G>
ZS_HD uint32_t png_pack_group_as(const PngPackImg &im, const uint32_t *table, int64_t y, int64_t rb, uint8_t *dst, int64_t b0) {
    static_assert(G == 4 || G == 8 || G == 16, "a group is one store");
    constexpr int CH = CT == 2 ? 3 : CT == 4 ? 2 : CT == 6 ? 4 : 1;
    // byte k of the group in bits 8k.. of v0 (k < 8) or v1: two scalars, not an array -- an array indexed by k would live in
    // scratch memory on the device
    uint64_t v0 = 0, v1 = 0;
    uint32_t miss = 0;
    const int64_t lo = b0 < 0 ? 0 : b0, hi = b0 + G < rb ? b0 + G : rb;  // the group's bytes inside the row
    const uint8_t *src = im.in + y * ((int64_t)im.width * png_expand_bytes(F));
    if constexpr (D < 8) {
        static_assert(G <= 8, "the sub-byte groups fit v0");
        constexpr int ppb = 8 / D;
        for (int64_t b = lo; b < hi; b++) {
            uint32_t byte = 0;
            for (int q = 0; q < ppb; q++) {
                const int64_t x = b * ppb + q;
                if (x >= im.width) break;  // (the unused low bits of the row's last byte stay zero)
                byte |= (uint32_t)png_pack_pixel<F, CT, D>(im, table, src, x, &miss) << (8 - D - q * D);
            }
            v0 |= (uint64_t)byte << (8 * (b - b0));
        }
    } else {
        // whole pixels of BPP bytes; the first and the last may lie partly in a neighbouring group
        constexpr int BPP = CH * D / 8;
        for (int64_t x = lo / BPP; x * BPP < hi; x++) {
            uint64_t px = png_pack_pixel<F, CT, D>(im, table, src, x, &miss);
            int o = (int)(x * BPP - b0);  // the pixel's first byte in the group: -7 .. G - 1
            if (o < 0) px >>= -8 * o, o = 0;
            if (o < 8) {
                v0 |= px << (8 * o);
                if (o > 0) v1 |= px >> (8 * (8 - o));
            } else
                v1 |= px << (8 * (o - 8));
        }
    }
    if (lo == b0 && hi == b0 + G) {
        const uint64_t v[2] = {v0, v1};
        __builtin_memcpy(__builtin_assume_aligned(dst + b0, G), v, G);
    } else
        for (int64_t b = lo; b < hi; b++) {
            const int k = (int)(b - b0);
            dst[b] = (uint8_t)((k < 8 ? v0 : v1) >> (8 * (k & 7)));
        }
    return miss;
}

// ... the (colour type, depth) pair is the same for a whole row: one jump, then straight code.  G: kAdam7GroupBits below 8
// bits a pixel (a lane reads 8 .. 32 source pixels for its 4 bytes), kPngPackGroup from there on.
template <int F>
ZS_HD uint32_t png_pack_group(const PngPackImg &im, const uint32_t *table, int64_t y, int64_t rb, uint8_t *dst, int64_t b0) {
    constexpr int GB = kAdam7GroupBits, GP = kPngPackGroup;
    switch (im.color * 32 + im.depth) {
    case 0 * 32 + 1: return png_pack_group_as<F, 0, 1, GB>(im, table, y, rb, dst, b0);
    case 0 * 32 + 2: return png_pack_group_as<F, 0, 2, GB>(im, table, y, rb, dst, b0);
    case 0 * 32 + 4: return png_pack_group_as<F, 0, 4, GB>(im, table, y, rb, dst, b0);
    case 0 * 32 + 8: return png_pack_group_as<F, 0, 8, GP>(im, table, y, rb, dst, b0);
    case 0 * 32 + 16: return png_pack_group_as<F, 0, 16, GP>(im, table, y, rb, dst, b0);
    case 2 * 32 + 8: return png_pack_group_as<F, 2, 8, GP>(im, table, y, rb, dst, b0);
    case 2 * 32 + 16: return png_pack_group_as<F, 2, 16, GP>(im, table, y, rb, dst, b0);
    case 3 * 32 + 1: return png_pack_group_as<F, 3, 1, GB>(im, table, y, rb, dst, b0);
    case 3 * 32 + 2: return png_pack_group_as<F, 3, 2, GB>(im, table, y, rb, dst, b0);
    case 3 * 32 + 4: return png_pack_group_as<F, 3, 4, GB>(im, table, y, rb, dst, b0);
    case 3 * 32 + 8: return png_pack_group_as<F, 3, 8, GP>(im, table, y, rb, dst, b0);
    case 4 * 32 + 8: return png_pack_group_as<F, 4, 8, GP>(im, table, y, rb, dst, b0);
    case 4 * 32 + 16: return png_pack_group_as<F, 4, 16, GP>(im, table, y, rb, dst, b0);
    case 6 * 32 + 8: return png_pack_group_as<F, 6, 8, GP>(im, table, y, rb, dst, b0);
    case 6 * 32 + 16: return png_pack_group_as<F, 6, 16, GP>(im, table, y, rb, dst, b0);
    default: return 0;  // (the host admits the fifteen pairs of table 11.1 only)
    }
}
ZS_HD constexpr int png_pack_group_bytes(int bits) { return bits < 8 ? kAdam7GroupBits : kPngPackGroup; }

// ---- the survey (KV, zs_png.hip): what an image's pixels allow ----
// A pixel's share of the violation mask, and its colour reduced to RGBA8 (meaningful where the pixel is low8).
constexpr uint32_t kSvNotOpaque = 1, kSvNotGray = 2, kSvNotLow8 = 4, kSvNot17 = 8, kSvNot85 = 16, kSvNot255 = 32, kSvWhite = 64;
constexpr int kSurveyRows = 16;       // rows of one image a workgroup of the first launch takes
constexpr int kSurveySlots = 1024;    // a workgroup's colour set: <= 257 counted and <= 256 on their way in, so never full
constexpr uint32_t kSurveyEmpty = 0xFFFFFFFFu;  // (that colour itself is kept as a bit of the mask: kSvWhite)
constexpr uint32_t kSurveyMany = 257;
struct PngSurveyImg {
    const uint8_t *in;   // height rows of row_pixels pixels, no padding, aligned to a pixel
    int64_t row_pixels;
    int32_t height, pad;
};
struct PngSurveyRec {
    uint32_t mask, count;  // count: colours in colors[] (the white of kSvWhite is not among them), or kSurveyMany
    uint32_t colors[256];
};
template <int F>
ZS_HD uint32_t png_survey_pixel(uint64_t raw, uint32_t *rgba8) {
    uint32_t m = 0, r, g, b, a;
    if constexpr (F == ZS_PNG_FMT_RGBA8) {
        r = (uint32_t)raw & 255, g = (uint32_t)raw >> 8 & 255, b = (uint32_t)raw >> 16 & 255, a = (uint32_t)raw >> 24;
        *rgba8 = (uint32_t)raw;
    } else {
        const uint32_t r16 = (uint32_t)raw & 0xFFFFu, g16 = (uint32_t)(raw >> 16) & 0xFFFFu, b16 = (uint32_t)(raw >> 32) & 0xFFFFu, a16 = (uint32_t)(raw >> 48);
        if (a16 != 0xFFFFu) m |= kSvNotOpaque;
        if (r16 != g16 || g16 != b16) m |= kSvNotGray;
        if (r16 % 257 || g16 % 257 || b16 % 257 || a16 % 257) m |= kSvNotLow8;
        r = r16 >> 8, g = g16 >> 8, b = b16 >> 8, a = a16 >> 8;
        *rgba8 = r | g << 8 | b << 16 | a << 24;
    }
    if constexpr (F == ZS_PNG_FMT_RGBA8) {
        if (a != 255) m |= kSvNotOpaque;
        if (r != g || g != b) m |= kSvNotGray;
    }
    if (r % 17 || g % 17 || b % 17) m |= kSvNot17;
    if (r % 85 || g % 85 || b % 85) m |= kSvNot85;
    if (r % 255 || g % 255 || b % 255) m |= kSvNot255;
    return m;
}

// ---- the choice of a file format from a survey (zs_png_choose_format): compares bits per pixel, nothing else ----
inline void png_choose_format(bool opaque, bool gray, bool low8, int sample_depth, int n_colors, int *color_type, int *bit_depth) {
    if (!low8) {
        *color_type = gray ? (opaque ? 0 : 4) : (opaque ? 2 : 6);
        *bit_depth = 16;
        return;
    }
    int ct = gray ? (opaque ? 0 : 4) : (opaque ? 2 : 6), bd = ct == 0 ? sample_depth : 8;
    const int base_bits = bd * (ct == 2 ? 3 : ct == 4 ? 2 : ct == 6 ? 4 : 1);
    if (n_colors <= 256) {
        const int p = n_colors <= 2 ? 1 : n_colors <= 4 ? 2 : n_colors <= 16 ? 4 : 8;
        if (p < base_bits) ct = 3, bd = p;  // (a tie keeps the base, which needs no PLTE)
    }
    *color_type = ct, *bit_depth = bd;
}

// ---- composing the frames of an animation (KM, zs_png.hip, and its host model tests/cpp/test_png_compose.cpp) ----
// Frame k of an animated PNG is a rectangle of RGBA pixels that is drawn onto a canvas; canvas k is what a viewer shows
// while frame k is up (APNG specification 1.0, "fcTL").  The canvas starts as transparent black.  A pixel is held as
// png_expand_pack makes it: RGBA8 in the low 32 bits (R lowest), RGBA16 as four uint16, R lowest.
//   blend SOURCE: the region takes the frame's pixels.
//   blend OVER, per pixel, M = 255 or 65535, foreground (f, fa), canvas (b, ba): fa == 0 leaves the canvas alone;
//     fa == M or ba == 0 copies the frame's pixel; otherwise u = fa * M, v = (M - fa) * ba, al = u + v, every colour channel
//     becomes (f * u + b * v) / al and alpha al / M, both floor divisions (64-bit products at RGBA16).  This is the integer
//     arithmetic of the specification's sample code.
//   dispose, after canvas k is written: NONE keeps the canvas; BACKGROUND sets the region to transparent black; PREVIOUS
//     puts back what the region held before frame k was drawn, and acts as BACKGROUND on frame 0.
constexpr int kPngComposeGroup = 16;  // canvas bytes a lane carries: 4 pixels of RGBA8, 2 of RGBA16

struct PngComposeFrame {
    const uint8_t *px;  // height rows of width * png_expand_bytes(format) bytes, aligned to a pixel
    int32_t x, y, width, height;  // the region: inside the canvas
    int32_t dispose, blend;
};
struct PngComposeAnim {
    uint8_t *out;  // n_frames canvases of height rows of width * png_expand_bytes(format) bytes, aligned to a pixel
    int32_t width, height;
    int32_t frame0, n_frames;  // its frames in the call's list of frames
};

// waves that share a canvas row: one per 64 groups
ZS_HD int64_t png_compose_row_waves(int64_t width, int format) {
    const int64_t n = kPngComposeGroup / png_expand_bytes(format), groups = (width + n - 1) / n;
    return (groups + 63) / 64;
}

template <int F>
ZS_HD uint32_t png_px_channel(uint64_t px, int k) {
    if constexpr (F == ZS_PNG_FMT_RGBA8) return (uint32_t)(px >> (8 * k)) & 255u;
    else return (uint32_t)(px >> (16 * k)) & 65535u;
}
template <int F>
ZS_HD uint64_t png_blend_over(uint64_t fg, uint64_t bg) {
    constexpr uint32_t M = F == ZS_PNG_FMT_RGBA8 ? 255u : 65535u;
    const uint32_t fa = png_px_channel<F>(fg, 3), ba = png_px_channel<F>(bg, 3);
    if (fa == 0) return bg;
    if (fa == M || ba == 0) return fg;
    const uint32_t u = fa * M, v = (M - fa) * ba, al = u + v;  // (al <= M * M < 2^32)
    uint32_t c[3];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 3; k++) {
        if constexpr (F == ZS_PNG_FMT_RGBA8) c[k] = (png_px_channel<F>(fg, k) * u + png_px_channel<F>(bg, k) * v) / al;
        else c[k] = (uint32_t)(((uint64_t)png_px_channel<F>(fg, k) * u + (uint64_t)png_px_channel<F>(bg, k) * v) / al);
    }
    return png_expand_pack<F>(c[0], c[1], c[2], al / M);
}
template <int F>
ZS_HD uint64_t png_compose_blend(int blend, uint64_t fg, uint64_t bg) {
    return blend == 0 ? fg : png_blend_over<F>(fg, bg);
}
// what a pixel of frame k's region holds once the frame's time is up: `shown` is canvas k's value, `before` the value in
// front of the frame's blend
ZS_HD uint64_t png_compose_dispose(int dispose, int k, uint64_t shown, uint64_t before) {
    return dispose == 0 ? shown : dispose == 2 && k > 0 ? before : 0;
}
template <int F>
ZS_HD uint64_t png_compose_load(const uint8_t *p) {
    if constexpr (F == ZS_PNG_FMT_RGBA8) {
        uint32_t v;
        __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
        return v;
    } else {
        uint64_t v;
        __builtin_memcpy(&v, __builtin_assume_aligned(p, 8), 8);
        return v;
    }
}

// Pixels [x0, x0 + N) of row y (N = 16 / pixel size; the part of them inside the row) in all of the animation's canvases:
// what one lane does.  The pixels' current values, and their values in front of the frame at hand, stay in
// registers through the frames; a frame's pixels are read only where (x, y) falls into its region, the row tested first
// (uniform over a wave); every canvas's pixels are stored once, as one 16-byte store where the group is whole and its
// address in that canvas is 16-aligned, pixel by pixel elsewhere.  No canvas byte is read, none is written twice.
template <int F>
ZS_HD void png_compose_group(const PngComposeAnim &a, const PngComposeFrame *frames, int64_t y, int64_t x0) {
    constexpr int P = png_expand_bytes(F), N = kPngComposeGroup / P;
    const int64_t rb = (int64_t)a.width * P, canvas = rb * a.height;
    const bool whole = x0 + N <= a.width;
    uint64_t cur[N], before[N];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < N; j++) cur[j] = 0, before[j] = 0;
    uint8_t *dst = a.out + y * rb + x0 * P;
    for (int k = 0; k < a.n_frames; k++, dst += canvas) {
        const PngComposeFrame fr = frames[a.frame0 + k];  // (a copy: the stores below do not make the compiler read it again)
        const bool row_in = y >= fr.y && y < (int64_t)fr.y + fr.height;
        bool in[N];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < N; j++) in[j] = false;
        if (row_in) {
            const int64_t fx = x0 - fr.x;  // the group's first column in the frame
            const uint8_t *src = fr.px + ((y - fr.y) * (int64_t)fr.width + fx) * P;
            uint64_t fg[N];
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int j = 0; j < N; j++) in[j] = fx + j >= 0 && fx + j < fr.width, fg[j] = 0;
            if (fx >= 0 && fx + N <= fr.width && ((uint64_t)(uintptr_t)src & (kPngComposeGroup - 1)) == 0) {
                uint64_t v[2];
                __builtin_memcpy(v, __builtin_assume_aligned(src, kPngComposeGroup), kPngComposeGroup);
                if constexpr (F == ZS_PNG_FMT_RGBA8) fg[0] = v[0] & 0xFFFFFFFFu, fg[1] = v[0] >> 32, fg[2] = v[1] & 0xFFFFFFFFu, fg[3] = v[1] >> 32;
                else fg[0] = v[0], fg[1] = v[1];
            } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
                for (int j = 0; j < N; j++)
                    if (in[j]) fg[j] = png_compose_load<F>(src + j * P);
            }
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int j = 0; j < N; j++)
                if (in[j]) before[j] = cur[j], cur[j] = png_compose_blend<F>(fr.blend, fg[j], cur[j]);
        }
        if (whole && ((uint64_t)(uintptr_t)dst & (kPngComposeGroup - 1)) == 0) {
            uint64_t v[2];
            if constexpr (F == ZS_PNG_FMT_RGBA8) v[0] = cur[0] | cur[1] << 32, v[1] = cur[2] | cur[3] << 32;
            else v[0] = cur[0], v[1] = cur[1];
            __builtin_memcpy(__builtin_assume_aligned(dst, kPngComposeGroup), v, kPngComposeGroup);
        } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int j = 0; j < N; j++)
                if (x0 + j < a.width) __builtin_memcpy(__builtin_assume_aligned(dst + j * P, P), &cur[j], P);
        }
        if (row_in) {
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int j = 0; j < N; j++)
                if (in[j]) cur[j] = png_compose_dispose(fr.dispose, k, cur[j], before[j]);
        }
    }
}

// ---- the frame diff (KD, zs_png.hip, and its host model tests/cpp/test_png_diff.cpp): KM's counterpart on the way out ----
// Frame f >= 1 of an animation that is written from its canvases is the smallest rectangle that holds every pixel whose
// bytes differ between canvas f - 1 and canvas f; drawn with blend SOURCE under dispose NONE it turns the one into the other.
// KD has KM's grid: a wave per stretch of 64 groups of a canvas row, a lane per group of 16 bytes, fixed by column.  The lane
// keeps canvas f - 1's group in registers and loads canvas f's (png_diff_load), so every canvas is read once; whether and
// where the two differ inside the group is png_diff_group; the wave's __ballot of "differs" gives the first and the last
// differing lane, and those two lanes' first / last differing pixel close the wave's record for the frame (png_diff_record):
// the differing columns of one stretch of one row.  A second launch folds a frame's records into its rectangle
// (png_diff_merge, png_diff_finish).
struct PngDiffAnim {
    const uint8_t *in;  // n_frames canvases of height rows of width * png_expand_bytes(format) bytes back to back, aligned to a pixel
    int64_t rec0;       // its first record: frame f's records are the waves' [rec0 + (f - 1) * waves, + waves)
    int32_t width, height;
    int32_t n_frames, pad;
};
struct PngDiffRec {
    int32_t x0, x1;  // the first and the last differing column of the stretch; x0 > x1: none
};
struct PngDiffRect {
    int32_t x0, y0, x1, y1;  // inclusive; x0 > x1: no pixel differs
};
ZS_HD PngDiffRec png_diff_none() { return PngDiffRec{0x7FFFFFFF, -1}; }
ZS_HD PngDiffRect png_diff_empty() { return PngDiffRect{0x7FFFFFFF, 0x7FFFFFFF, -1, -1}; }

// The group of pixels [x0, x0 + N) of a canvas row, `p` its first pixel: one 16-byte load where the group is whole and the
// address allows, pixel loads elsewhere (a canvas whose size is no multiple of 16 shifts every later canvas's alignment).
// Pixels beyond the row are zero.  Nothing outside the row is read.
template <int F>
ZS_HD void png_diff_load(const uint8_t *p, int64_t x0, int64_t width, uint64_t v[2]) {
    constexpr int P = png_expand_bytes(F), N = kPngComposeGroup / P;
    if (x0 + N <= width && ((uint64_t)(uintptr_t)p & (kPngComposeGroup - 1)) == 0) {
        __builtin_memcpy(v, __builtin_assume_aligned(p, kPngComposeGroup), kPngComposeGroup);
        return;
    }
    v[0] = 0, v[1] = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < N; j++)
        if (x0 + j < width) {
            const uint64_t px = png_compose_load<F>(p + j * P);
            if constexpr (F == ZS_PNG_FMT_RGBA8) v[j >> 1] |= px << (32 * (j & 1));
            else v[j] = px;
        }
}

// Do the two groups differ in any byte, and if so, which are the first and the last differing pixel (0 .. N - 1)?
template <int F>
ZS_HD bool png_diff_group(const uint64_t a[2], const uint64_t b[2], int *first, int *last) {
    const uint64_t d0 = a[0] ^ b[0], d1 = a[1] ^ b[1];
    if ((d0 | d1) == 0) return false;
    if constexpr (F == ZS_PNG_FMT_RGBA8) {
        const uint32_t m = ((uint32_t)d0 != 0 ? 1u : 0u) | ((d0 >> 32) != 0 ? 2u : 0u) | ((uint32_t)d1 != 0 ? 4u : 0u) | ((d1 >> 32) != 0 ? 8u : 0u);
        *first = __builtin_ctz(m), *last = 31 - __builtin_clz(m);
    } else {
        *first = d0 ? 0 : 1, *last = d1 ? 1 : 0;
    }
    return true;
}
// the first and the last set lane of a wave's ballot (mask != 0)
ZS_HD int png_diff_first_lane(uint64_t mask) { return __builtin_ctzll(mask); }
ZS_HD int png_diff_last_lane(uint64_t mask) { return 63 - __builtin_clzll(mask); }
// The wave's record: lanes lo and hi are the first and the last whose group differs, `first_lo` and `last_hi` what
// png_diff_group gave those two; g0 is the stretch's first group and n the pixels of a group.
ZS_HD PngDiffRec png_diff_record(int lo, int hi, int64_t g0, int n, int first_lo, int last_hi) {
    return PngDiffRec{(int32_t)((g0 + lo) * n + first_lo), (int32_t)((g0 + hi) * n + last_hi)};
}
// a record of row y folded into a rectangle; two rectangles folded into one
ZS_HD PngDiffRect png_diff_merge(PngDiffRect r, PngDiffRec c, int32_t y) {
    if (c.x0 > c.x1) return r;
    return PngDiffRect{c.x0 < r.x0 ? c.x0 : r.x0, y < r.y0 ? y : r.y0, c.x1 > r.x1 ? c.x1 : r.x1, y > r.y1 ? y : r.y1};
}
ZS_HD PngDiffRect png_diff_union(PngDiffRect a, PngDiffRect b) {
    return PngDiffRect{a.x0 < b.x0 ? a.x0 : b.x0, a.y0 < b.y0 ? a.y0 : b.y0, a.x1 > b.x1 ? a.x1 : b.x1, a.y1 > b.y1 ? a.y1 : b.y1};
}
// ... and the frame's region: APNG has no empty frame, so no difference is the 1 x 1 rectangle at (0, 0)
ZS_HD void png_diff_finish(PngDiffRect r, int64_t *x, int64_t *y, int64_t *width, int64_t *height) {
    if (r.x0 > r.x1) *x = 0, *y = 0, *width = 1, *height = 1;
    else *x = r.x0, *y = r.y0, *width = (int64_t)r.x1 - r.x0 + 1, *height = (int64_t)r.y1 - r.y0 + 1;
}

// ---- the crop (zs_png.hip zs_png_crop_kernel): a rectangle of an image as tight rows ----
struct PngCropImg {
    const uint8_t *in;  // the rectangle's first pixel in the image, aligned to a pixel
    uint8_t *out;       // height rows of width * P bytes, aligned to a pixel
    int64_t in_pitch;   // bytes from one image row to the next
    int32_t width, height;
};
// Bytes [b0, b0 + 16) of output row y (`dst` = the row's first byte, `rb` its length; dst + b0 is 16-aligned, and dst is
// aligned to a pixel of P bytes, so a group holds whole pixels).  A whole group is one 16-byte store, fed by one 16-byte
// load where source and destination agree modulo 16 and by pixel loads elsewhere; the ragged first and last group of a row
// go pixel by pixel.  No byte outside the row is touched, in or out.
template <int P>
ZS_HD void png_crop_group(const PngCropImg &im, int64_t y, int64_t rb, uint8_t *dst, int64_t b0) {
    static_assert(P == 4 || P == 8, "a pixel is RGBA8 or RGBA16");
    const int64_t lo = b0 < 0 ? 0 : b0, hi = b0 + 16 < rb ? b0 + 16 : rb;
    const uint8_t *src = im.in + y * im.in_pitch;
    if (lo == b0 && hi == b0 + 16) {
        uint64_t v[2];
        if (((uint64_t)(uintptr_t)(src + b0) & 15) == 0) __builtin_memcpy(v, __builtin_assume_aligned(src + b0, 16), 16);
        else if constexpr (P == 8) {
            __builtin_memcpy(&v[0], __builtin_assume_aligned(src + b0, 8), 8);
            __builtin_memcpy(&v[1], __builtin_assume_aligned(src + b0 + 8, 8), 8);
        } else {
            uint32_t w[4];
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int j = 0; j < 4; j++) __builtin_memcpy(&w[j], __builtin_assume_aligned(src + b0 + 4 * j, 4), 4);
            v[0] = w[0] | (uint64_t)w[1] << 32, v[1] = w[2] | (uint64_t)w[3] << 32;
        }
        __builtin_memcpy(__builtin_assume_aligned(dst + b0, 16), v, 16);
    } else
        for (int64_t b = lo; b < hi; b += P) {
            uint64_t px = 0;
            __builtin_memcpy(&px, __builtin_assume_aligned(src + b, P), P);
            __builtin_memcpy(__builtin_assume_aligned(dst + b, P), &px, P);
        }
}


}  // namespace zs
