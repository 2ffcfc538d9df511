// test_png_adam7_split.cpp -- the gather of the Adam7 split kernel (zlibstream_amd/csrc/zs_png.hip, KS) run on the host with
// the code the kernel compiles (zs_png.h): the descriptor's layout, the map from a flat pass row to its pass, and the aligned
// groups of output bytes a lane builds and stores -- at every group width the kernel is built for, with the source and the
// destination at every byte residue mod 16.  Compared with a plain restatement of the table of PNG specification 8.2 written
// here: nested loops over xstart + k * xstep, sub-byte packing, zero padding bits.  The source's padding bits are all ones
// (the specification leaves them unspecified: none may reach the output); the destination starts poisoned and has guard bytes
// on both sides, so a byte not written, or written outside, shows.  The result then goes through KA's code (adam7_group):
// the original rows come back, padding bits cleared.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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

// a random image whose rows' padding bits are ones, the passes it splits into (back to back, absent ones absent, padding bits
// zero), the same image with its padding bits cleared, and the pass rows there are
void reference(int w, int h, int bits, std::mt19937 &rng, std::vector<uint8_t> &image, std::vector<uint8_t> &passes, std::vector<uint8_t> &cleared,
               int64_t *pass_rows) {
    const int64_t rb = ((int64_t)w * bits + 7) / 8;
    image.resize((size_t)(rb * h));
    for (auto &b : image) b = (uint8_t)rng();
    cleared = image;
    const int used = (int)(((int64_t)w * bits) % 8);
    if (used)
        for (int y = 0; y < h; y++) {
            image[(size_t)(y * rb + rb - 1)] |= (uint8_t)(0xFF >> used);
            cleared[(size_t)(y * rb + rb - 1)] &= (uint8_t)~(0xFF >> used);
        }
    passes.clear();
    *pass_rows = 0;
    for (int p = 0; p < 7; p++) {
        int64_t pw = 0, ph = 0;
        for (int x = kXStart[p]; x < w; x += kXStep[p]) pw++;
        for (int y = kYStart[p]; y < h; y += kYStep[p]) ph++;
        if (pw == 0 || ph == 0) continue;
        *pass_rows += ph;
        const int64_t prb = (pw * bits + 7) / 8;
        const size_t at = passes.size();
        passes.resize(at + (size_t)(prb * ph), 0);
        int64_t j = 0;
        for (int y = kYStart[p]; y < h; y += kYStep[p], j++) {
            int64_t k = 0;
            for (int x = kXStart[p]; x < w; x += kXStep[p], k++) {
                uint8_t px[8];
                const int v = get_px(&image[(size_t)(y * rb)], x, bits, px);
                put_px(&passes[at + (size_t)(j * prb)], k, bits, v, px);
            }
        }
    }
}

long n_cases = 0;

uint8_t *aligned16(std::vector<uint8_t> &buf) {
    uint8_t *p = buf.data();
    return p + ((16 - ((uintptr_t)p & 15)) & 15);
}

// the kernel's loop: per flat pass row its pass, then the groups that cover the row, every group by one lane; then KA's loop
// over the result
template <int G>
bool split_model(int w, int h, int bits, const std::vector<uint8_t> &image, const std::vector<uint8_t> &want, const std::vector<uint8_t> &cleared, int64_t pass_rows,
                 int src_align, int dst_align) {
    const size_t guard = 64;
    // the source ends where its allocation ends: a read behind it is an error under a sanitizer
    void *smem = nullptr;
    if (posix_memalign(&smem, 16, (size_t)src_align + image.size()) != 0) return printf("FAIL: no memory\n"), false;
    struct Free {
        void *p;
        ~Free() { free(p); }
    } sfree{smem};
    uint8_t *src = (uint8_t *)smem + src_align;
    memset(smem, 0xFF, (size_t)src_align);
    memcpy(src, image.data(), image.size());
    std::vector<uint8_t> dbuf(16 + guard + 16 + want.size() + guard, 0xEE);
    uint8_t *out = aligned16(dbuf) + guard + dst_align;
    Adam7SplitImg im{src, out, {}, {}, w, h, bits, 0};
    if (adam7_split_layout(im) != (int64_t)want.size()) return printf("FAIL: layout bytes\n"), false;
    if (im.row0[kAdam7Passes] != pass_rows || adam7_pass_rows(w, h) != pass_rows) return printf("FAIL: pass rows\n"), false;
    for (int64_t r = 0; r < pass_rows; r++) {
        const int p = adam7_split_pass(im, r);
        const int64_t j = r - im.row0[p], pw = adam7_pass_width(w, p), prb = png_bits_row_bytes(pw, bits);
        if (j < 0 || j >= adam7_pass_height(h, p) || pw <= 0) return printf("FAIL: pass row %ld is row %ld of pass %d\n", (long)r, (long)j, p + 1), false;
        uint8_t *dst = im.passes + im.off[p] + j * prb;
        const uint64_t addr = (uint64_t)(uintptr_t)dst;
        if (bits < 8 && p != 6) {
            const int64_t ng = adam7_row_groups(addr, prb, kAdam7GroupBits), b0 = adam7_row_b0(addr, kAdam7GroupBits);
            for (int64_t g = 0; g < ng; g++) adam7_split_group<kAdam7GroupBits>(im, p, j, prb, dst, b0 + g * kAdam7GroupBits);
        } else {
            const int64_t ng = adam7_row_groups(addr, prb, G), b0 = adam7_row_b0(addr, G);
            for (int64_t g = 0; g < ng; g++) adam7_split_group<G>(im, p, j, prb, dst, b0 + g * G);
        }
    }
    n_cases++;
    if (memcmp(out, want.data(), want.size()) != 0) return printf("FAIL: the passes differ\n"), false;
    for (uint8_t *q = dbuf.data(); q < out; q++)
        if (*q != 0xEE) return printf("FAIL: a byte in front of the passes was written\n"), false;
    for (uint8_t *q = out + want.size(); q < dbuf.data() + dbuf.size(); q++)
        if (*q != 0xEE) return printf("FAIL: a byte behind the passes was written\n"), false;
    if (memcmp(src, image.data(), image.size()) != 0) return printf("FAIL: the source changed\n"), false;
    // back through KA's code: the original rows, padding bits cleared
    const int64_t rb = png_bits_row_bytes(w, bits);
    std::vector<uint8_t> back(16 + (size_t)(rb * h) + 16, 0xEE);
    Adam7Img mi{out, aligned16(back), {}, w, h, bits, 0};
    adam7_layout(mi);
    for (int64_t y = 0; y < h; y++) {
        uint8_t *dst = mi.out + y * rb;
        const uint64_t addr = (uint64_t)(uintptr_t)dst;
        const int64_t ng = adam7_row_groups(addr, rb, 4), b0 = adam7_row_b0(addr, 4);
        for (int64_t g = 0; g < ng; g++) adam7_group<4>(mi, y, rb, dst, b0 + g * 4);
    }
    if (memcmp(mi.out, cleared.data(), cleared.size()) != 0) return printf("FAIL: the merge of the split is not the image\n"), false;
    return true;
}

bool one_shape(int w, int h, int bits, std::mt19937 &rng) {
    std::vector<uint8_t> image, want, cleared;
    int64_t pass_rows = 0;
    reference(w, h, bits, rng, image, want, cleared, &pass_rows);
    // source and destination at every residue mod 16: each against a few of the other's, all of both covered
    for (int a = 0; a < 16; a++) {
        const int others[3] = {a, (a * 7 + 3) & 15, (15 - a)};
        for (int b : others) {
            if (!split_model<4>(w, h, bits, image, want, cleared, pass_rows, a, b) || !split_model<8>(w, h, bits, image, want, cleared, pass_rows, b, a) ||
                !split_model<16>(w, h, bits, image, want, cleared, pass_rows, a, b))
                return printf("FAIL: split %dx%d @%d bits, residues %d / %d\n", w, h, bits, a, b), false;
        }
    }
    return true;
}

}  // namespace

int main() {
    std::mt19937 rng(20261019u);
    const int depths[] = {1, 2, 4, 8, 16, 24, 32, 48, 64};
    for (int bits : depths) {
        for (int w = 1; w <= 20; w++)
            for (int h = 1; h <= 20; h++)
                if (!one_shape(w, h, bits, rng)) return 1;
        if (!one_shape(1000, 3, bits, rng) || !one_shape(257, 63, bits, rng) || !one_shape(33, 31, bits, rng) || !one_shape(65, 129, bits, rng)) return 1;
    }
    printf("PASS %ld splits\n", n_cases);
    return 0;
}
