// test_png_adam7.cpp -- the Adam7 geometry and the gather of the interleave kernel (zlibstream_amd/csrc/zs_png.hip, KA) run
// on the host with the code the kernel compiles (zs_png.h): the pass sizes, the inverse map from an output pixel to its pass
// and place, and the aligned groups of output bytes a lane builds and stores -- at every group width the kernel is built
// for and with the output row at every byte alignment.  Compared with a plain restatement of the table of PNG
// specification 8.2 written here: nested loops over xstart + k * xstep, sub-byte packing, zero padding bits.
// The output starts poisoned and has guard bytes on both sides: a byte not written, or written outside, shows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_png.h"

using namespace zs;

namespace {

// PNG specification 8.2, copied from the document and not from zs_png.h
const int kXStart[7] = {0, 4, 0, 2, 0, 1, 0}, kYStart[7] = {0, 0, 4, 0, 2, 0, 1};
const int kXStep[7] = {8, 8, 4, 4, 2, 2, 1}, kYStep[7] = {8, 8, 8, 4, 4, 2, 2};

int get_px(const uint8_t *row, int64_t x, int bits, uint8_t *bytes) {  // sub-byte: the value; else the pixel's bytes
    if (bits < 8) return (row[x * bits / 8] >> (8 - bits - (x * bits) % 8)) & ((1 << bits) - 1);
    memcpy(bytes, row + x * (bits / 8), (size_t)(bits / 8));
    return 0;
}
void put_px(uint8_t *row, int64_t x, int bits, int v, const uint8_t *bytes) {
    if (bits < 8) row[x * bits / 8] |= (uint8_t)(v << (8 - bits - (x * bits) % 8));
    else memcpy(row + x * (bits / 8), bytes, (size_t)(bits / 8));
}

// the passes of an image back to back (random pixels; the padding bits of a pass row random too: the merge must not carry
// them over), and the image they interleave to
void reference(int w, int h, int bits, std::mt19937 &rng, std::vector<uint8_t> &passes, std::vector<uint8_t> &image, int64_t pass_px[7]) {
    const int64_t rb = ((int64_t)w * bits + 7) / 8;
    image.assign((size_t)(rb * h), 0);
    passes.clear();
    for (int p = 0; p < 7; p++) {
        int64_t pw = 0, ph = 0;
        for (int x = kXStart[p]; x < w; x += kXStep[p]) pw++;
        for (int y = kYStart[p]; y < h; y += kYStep[p]) ph++;
        pass_px[p] = pw * ph;
        if (pw == 0 || ph == 0) {
            pass_px[p] = 0;
            continue;
        }
        const int64_t prb = (pw * bits + 7) / 8;
        const size_t at = passes.size();
        passes.resize(at + (size_t)(prb * ph));
        for (size_t i = at; i < passes.size(); i++) passes[i] = (uint8_t)rng();
        int64_t j = 0;
        for (int y = kYStart[p]; y < h; y += kYStep[p], j++) {
            int64_t k = 0;
            for (int x = kXStart[p]; x < w; x += kXStep[p], k++) {
                uint8_t px[8];
                const int v = get_px(&passes[at + (size_t)(j * prb)], k, bits, px);
                put_px(&image[(size_t)(y * rb)], x, bits, v, px);
            }
        }
    }
}

long n_cases = 0;

template <int G>
bool merge_model(const Adam7Img &im0, int64_t rb, const std::vector<uint8_t> &want, int align, int group_bits) {
    // the kernel's loop: per row the groups that cover it, every group by one lane
    const size_t guard = 64;
    std::vector<uint8_t> buf(guard + (size_t)align + want.size() + guard + 16, 0xEE);
    uint8_t *base = buf.data();
    base += (16 - ((uintptr_t)base & 15)) & 15;  // 16-aligned, then the misalignment under test
    uint8_t *out = base + 32 + align;
    Adam7Img im = im0;
    im.out = out;
    for (int64_t y = 0; y < im.height; y++) {
        uint8_t *dst = im.out + y * rb;
        const uint64_t addr = (uint64_t)(uintptr_t)dst;
        if (im.bits < 8) {
            const int64_t ng = adam7_row_groups(addr, rb, group_bits), b0 = adam7_row_b0(addr, group_bits);
            for (int64_t g = 0; g < ng; g++) adam7_group<kAdam7GroupBits>(im, y, rb, dst, b0 + g * group_bits);
        } else {
            const int64_t ng = adam7_row_groups(addr, rb, G), b0 = adam7_row_b0(addr, G);
            for (int64_t g = 0; g < ng; g++) adam7_group<G>(im, y, rb, dst, b0 + g * G);
        }
    }
    n_cases++;
    if (memcmp(out, want.data(), want.size()) != 0) return false;
    for (uint8_t *p = buf.data(); p < out; p++)
        if (*p != 0xEE) return false;
    for (uint8_t *p = out + want.size(); p < buf.data() + buf.size(); p++)
        if (*p != 0xEE) return false;
    return true;
}

bool one_shape(int w, int h, int bits, std::mt19937 &rng) {
    std::vector<uint8_t> passes, want;
    int64_t pass_px[7];
    reference(w, h, bits, rng, passes, want, pass_px);
    const int64_t rb = png_bits_row_bytes(w, bits);
    if (rb != ((int64_t)w * bits + 7) / 8) return printf("FAIL: row bytes %dx%d @%d\n", w, h, bits), false;
    // the pass sizes: the table's, and together the image's pixels
    int64_t sum = 0, bytes = 0;
    Adam7Img im{passes.data(), nullptr, {}, w, h, bits, 0};
    for (int p = 0; p < kAdam7Passes; p++) {
        const int64_t pw = adam7_pass_width(w, p), ph = adam7_pass_height(h, p);
        if ((pw > 0 && ph > 0 ? pw * ph : 0) != pass_px[p]) return printf("FAIL: pass %d size %dx%d\n", p + 1, w, h), false;
        if (pw > 0 && ph > 0) sum += pw * ph, bytes += png_bits_row_bytes(pw, bits) * ph;
    }
    if (sum != (int64_t)w * h) return printf("FAIL: passes hold %ld pixels of %dx%d\n", (long)sum, w, h), false;
    if (adam7_layout(im) != bytes || bytes != (int64_t)passes.size()) return printf("FAIL: layout %dx%d @%d\n", w, h, bits), false;
    // the inverse map: onto the present passes' pixels, each exactly once
    if (bits == 8 || (w > 20 && bits == 1)) {
        std::set<std::vector<int64_t>> seen;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const Adam7Src s = adam7_source(x, y);
                if (s.pass < 0 || s.pass > 6 || s.col < 0 || s.col >= adam7_pass_width(w, s.pass) || s.row < 0 || s.row >= adam7_pass_height(h, s.pass))
                    return printf("FAIL: source of (%d, %d) outside its pass\n", x, y), false;
                if (kXStart[s.pass] + s.col * kXStep[s.pass] != x || kYStart[s.pass] + s.row * kYStep[s.pass] != y)
                    return printf("FAIL: source of (%d, %d) is another pixel\n", x, y), false;
                if (!seen.insert({s.pass, s.col, s.row}).second) return printf("FAIL: source of (%d, %d) taken twice\n", x, y), false;
            }
        if ((int64_t)seen.size() != sum) return printf("FAIL: not a bijection %dx%d\n", w, h), false;
    }
    // the gather, at every group width and the row start at every alignment of the widest group
    for (int align = 0; align < 16; align++) {
        if (w > 20 && align % 5 != 1) continue;  // (the larger shapes: alignments 1, 6, 11)
        if (!merge_model<4>(im, rb, want, align, kAdam7GroupBits) || !merge_model<8>(im, rb, want, align, kAdam7GroupBits) ||
            !merge_model<16>(im, rb, want, align, kAdam7GroupBits))
            return printf("FAIL: merge %dx%d @%d bits, alignment %d\n", w, h, bits, align), false;
    }
    return true;
}

}  // namespace

int main() {
    std::mt19937 rng(20261017u);
    const int depths[] = {1, 2, 4, 8, 16, 24, 32, 48, 64};
    for (int bits : depths) {
        if (!png_bits_ok(bits)) return printf("FAIL: %d bits rejected\n", bits), 1;
        for (int w = 1; w <= 20; w++)
            for (int h = 1; h <= 20; h++)
                if (!one_shape(w, h, bits, rng)) return 1;
        if (!one_shape(1000, 3, bits, rng) || !one_shape(257, 63, bits, rng)) return 1;
    }
    for (int bits = -1; bits <= 72; bits++) {
        bool in_set = false;
        for (int d : depths) in_set = in_set || d == bits;
        if (png_bits_ok(bits) != in_set) return printf("FAIL: png_bits_ok(%d)\n", bits), 1;
    }
    // the rows' sources as DESIGN.md states them
    for (int y = 0; y < 16; y++) {
        unsigned mask = 0;
        for (int x = 0; x < 16; x++) mask |= 1u << adam7_source(x, y).pass;
        const unsigned want = y % 2 ? 0x40u : y % 4 == 2 ? 0x30u : y % 8 == 4 ? 0x2Cu : 0x2Bu;
        if (mask != want) return printf("FAIL: row %d draws on passes %x\n", y, mask), 1;
    }
    printf("PASS %ld merges\n", n_cases);
    return 0;
}
