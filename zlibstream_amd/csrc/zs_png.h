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

}  // namespace zs
