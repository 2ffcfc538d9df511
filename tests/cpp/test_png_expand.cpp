// test_png_expand.cpp -- the expansion of raw PNG scanlines to RGBA8 / RGBA16 (zlibstream_amd/csrc/zs_png.hip, KX) run on the
// host with the code the kernel compiles (zs_png.h png_expand_group): whole rows, group by group as a wave's lanes take
// them, at all fifteen (colour type, bit depth) pairs, both formats, with the output row at every legal residue modulo 16.
// Compared with a per-pixel restatement of the rules written here from the PNG specification: divisions where the header
// multiplies, PLTE and tRNS looked up directly where the header reads a table.
// The input buffers are exactly as long as the image (a read outside shows under -fsanitize=address); the output starts
// poisoned and has guard bytes on both sides: a byte not written, or written outside, shows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_png.h"

using namespace zs;

namespace {

const int kPairs[15][2] = {{0, 1}, {0, 2}, {0, 4}, {0, 8}, {0, 16}, {2, 8}, {2, 16}, {3, 1}, {3, 2}, {3, 4}, {3, 8}, {4, 8}, {4, 16}, {6, 8}, {6, 16}};
int channels(int ct) { return ct == 2 ? 3 : ct == 4 ? 2 : ct == 6 ? 4 : 1; }

struct Image {
    int w, h, ct, d;
    std::vector<uint8_t> data;  // h rows of ceil(w * d * channels / 8) bytes
    std::vector<uint8_t> plte, trns;
};

int64_t row_bytes(const Image &im) { return ((int64_t)im.w * im.d * channels(im.ct) + 7) / 8; }

// sample k of pixel (x, y) at its original depth
uint32_t sample(const Image &im, int x, int y, int k) {
    const uint8_t *row = im.data.data() + y * row_bytes(im);
    const int ch = channels(im.ct);
    if (im.d == 16) return (uint32_t)row[(x * ch + k) * 2] * 256 + row[(x * ch + k) * 2 + 1];
    if (im.d == 8) return row[x * ch + k];
    const int per = 8 / im.d, shift = (per - 1 - x % per) * im.d;  // leftmost pixel in the high bits
    return (row[x / per] >> shift) % (1u << im.d);
}
void put_sample(Image &im, int x, int y, int k, uint32_t v) {
    uint8_t *row = im.data.data() + y * row_bytes(im);
    const int ch = channels(im.ct);
    if (im.d == 16) row[(x * ch + k) * 2] = (uint8_t)(v >> 8), row[(x * ch + k) * 2 + 1] = (uint8_t)v;
    else if (im.d == 8) row[x * ch + k] = (uint8_t)v;
    else {
        const int per = 8 / im.d, shift = (per - 1 - x % per) * im.d;
        row[x / per] = (uint8_t)((row[x / per] & ~(((1u << im.d) - 1) << shift)) | v << shift);
    }
}

// The rules, per pixel.  target: 8 or 16 bits a channel.
uint32_t scale(uint32_t v, int d, int target) {
    const uint32_t from = (1u << d) - 1, to = (1u << target) - 1;
    if (d == target) return v;
    if (d < target) return v * to / from;  // (exact: 2^d - 1 divides 2^target - 1 for d = 1, 2, 4, 8 and target 8, 16)
    return (v * 255 + 32895) >> 16;        // 16 to 8
}
void restate(const Image &im, int x, int y, int target, uint32_t rgba[4]) {
    const uint32_t top = (1u << target) - 1;
    if (im.ct == 3) {
        const uint32_t k = sample(im, x, y, 0), entries = (uint32_t)im.plte.size() / 3;
        for (int j = 0; j < 3; j++) rgba[j] = k < entries ? im.plte[3 * k + j] : 0;
        rgba[3] = k < entries && k < im.trns.size() ? im.trns[k] : 255;
        if (target == 16)
            for (int j = 0; j < 4; j++) rgba[j] *= 257;
        return;
    }
    const int ch = channels(im.ct), colors = ch >= 3 ? 3 : 1;
    for (int j = 0; j < 3; j++) rgba[j] = scale(sample(im, x, y, colors == 3 ? j : 0), im.d, target);
    if (ch == 2 || ch == 4) rgba[3] = scale(sample(im, x, y, ch - 1), im.d, target);
    else if (im.trns.empty()) rgba[3] = top;
    else {
        bool same = true;
        for (int j = 0; j < colors; j++) {
            const uint32_t key = (uint32_t)im.trns[2 * j] * 256 + im.trns[2 * j + 1];
            same = same && sample(im, x, y, j) == key % (1u << im.d);
        }
        rgba[3] = same ? 0 : top;
    }
}

long g_cases = 0, g_keyed = 0, g_beyond = 0;

bool run_case(const Image &im, int format, int residue) {
    const int P = png_expand_bytes(format), target = format == ZS_PNG_FMT_RGBA8 ? 8 : 16;
    const int64_t rb = (int64_t)im.w * P, total = rb * im.h;
    constexpr int kGuard = 64;
    std::vector<uint8_t> buf((size_t)(total + 2 * kGuard + 32), 0xA5);
    uint8_t *base = buf.data() + kGuard;
    base += (16 - (uintptr_t)base % 16) % 16 + residue;  // the first row's residue; the others follow from the row length

    std::vector<uint32_t> tables(3 * kPngPalEntries, 0x12345678u);  // the image's table is the second of three
    PngExpandImg d{im.data.data(), base, im.w, im.h, im.d, im.ct, format, 0, {0, 0, 0}, 0};
    if (im.ct == 3) {
        d.pal_off = kPngPalEntries;
        png_expand_table(im.plte.data(), (int)im.plte.size() / 3, im.trns.data(), (int)im.trns.size(), tables.data() + d.pal_off);
    } else if (!im.trns.empty()) {
        for (int j = 0; j < (im.ct == 0 ? 1 : 3); j++) d.key[j] = (uint16_t)(im.trns[2 * j] * 256 + im.trns[2 * j + 1]);
        d.has_key = 1;
    }
    for (int y = 0; y < im.h; y++) {
        uint8_t *dst = base + y * rb;
        const uint64_t addr = (uint64_t)(uintptr_t)dst;
        const int64_t ng = adam7_row_groups(addr, rb, kPngExpandGroup), b0 = adam7_row_b0(addr, kPngExpandGroup);
        // (the lanes of a wave in any order: no group depends on another)
        for (int64_t g = ng - 1; g >= 0; g--) {
            if (format == ZS_PNG_FMT_RGBA8) png_expand_group<ZS_PNG_FMT_RGBA8>(d, tables.data() + d.pal_off, y, dst, b0 + g * kPngExpandGroup);
            else png_expand_group<ZS_PNG_FMT_RGBA16>(d, tables.data() + d.pal_off, y, dst, b0 + g * kPngExpandGroup);
        }
    }
    for (uint8_t *p = buf.data(); p < buf.data() + buf.size(); p++)
        if ((p < base || p >= base + total) && *p != 0xA5) {
            printf("FAIL guard: type %d depth %d format %d %dx%d residue %d: byte %td of the buffer (row data is %td .. %td)\n", im.ct, im.d, format, im.w,
                   im.h, residue, p - buf.data(), base - buf.data(), base + total - buf.data());
            return false;
        }
    for (int y = 0; y < im.h; y++)
        for (int x = 0; x < im.w; x++) {
            uint32_t want[4], got[4];
            restate(im, x, y, target, want);
            const uint8_t *p = base + y * rb + (int64_t)x * P;
            for (int j = 0; j < 4; j++) {
                if (format == ZS_PNG_FMT_RGBA8) got[j] = p[j];
                else {
                    uint16_t v;
                    memcpy(&v, p + 2 * j, 2);
                    got[j] = v;
                }
            }
            if (memcmp(want, got, sizeof want) != 0) {
                printf("FAIL type %d depth %d format %d %dx%d residue %d trns %zu plte %zu: pixel (%d, %d) is %u %u %u %u, expected %u %u %u %u\n", im.ct, im.d,
                       format, im.w, im.h, residue, im.trns.size(), im.plte.size() / 3, x, y, got[0], got[1], got[2], got[3], want[0], want[1], want[2], want[3]);
                return false;
            }
            if (im.ct != 3 && !im.trns.empty() && want[3] == 0) g_keyed++;
            if (im.ct == 3 && sample(im, x, y, 0) >= im.plte.size() / 3) g_beyond++;
        }
    g_cases++;
    return true;
}

}  // namespace

int main() {
    std::mt19937 rng(20240607);
    std::vector<int> widths;
    for (int w = 1; w <= 70; w++) widths.push_back(w);
    for (int w : {255, 256, 257, 513}) widths.push_back(w);
    const int kEntries[5] = {1, 2, 16, 255, 256};
    int pal_turn = 0;
    for (const auto &pair : kPairs)
        for (int w : widths)
            for (int h : {1, 3})
                for (int with_trns = 0; with_trns < 2; with_trns++) {
                    Image im{w, h, pair[0], pair[1], {}, {}, {}};
                    im.data.resize((size_t)(row_bytes(im) * h));
                    for (auto &b : im.data) b = (uint8_t)rng();
                    const uint32_t mask = (1u << im.d) - 1;
                    if (im.ct == 3) {
                        const int entries = kEntries[pal_turn++ % 5];
                        im.plte.resize((size_t)entries * 3);
                        for (auto &b : im.plte) b = (uint8_t)rng();
                        if (with_trns) {
                            im.trns.resize((size_t)(1 + rng() % (unsigned)entries));
                            for (auto &b : im.trns) b = (uint8_t)rng();
                        }
                    } else if (with_trns && (im.ct == 0 || im.ct == 2)) {
                        // the key: the samples of one pixel of the image, with bits above the depth set in the chunk (they do not
                        // count); that pixel again elsewhere, and pixels that differ from it in one sample or one bit only
                        const int colors = im.ct == 0 ? 1 : 3, kx = (int)(rng() % (unsigned)w), ky = (int)(rng() % (unsigned)h);
                        uint32_t key[3];
                        im.trns.resize((size_t)colors * 2);
                        for (int j = 0; j < colors; j++) {
                            key[j] = sample(im, kx, ky, j);
                            const uint32_t stored = im.d < 16 ? key[j] | ((uint32_t)rng() & 0xFFFFu & ~mask) : key[j];
                            im.trns[2 * (size_t)j] = (uint8_t)(stored >> 8), im.trns[2 * (size_t)j + 1] = (uint8_t)stored;
                        }
                        for (int t = 0; t < 1 + w * h / 6; t++) {
                            const int x = (int)(rng() % (unsigned)w), y = (int)(rng() % (unsigned)h);
                            for (int j = 0; j < colors; j++) put_sample(im, x, y, j, key[j]);
                            const int x2 = (int)(rng() % (unsigned)w), y2 = (int)(rng() % (unsigned)h);
                            if (x2 == kx && y2 == ky) continue;
                            for (int j = 0; j < colors; j++) put_sample(im, x2, y2, j, key[j]);
                            const int which = (int)(rng() % (unsigned)colors);
                            // (at 16 bits: the same low byte, another high byte -- only the whole value counts)
                            put_sample(im, x2, y2, which, (key[which] ^ (im.d == 16 ? 0x0100u : 1u << (rng() % (unsigned)im.d))) & mask);
                        }
                    } else if (with_trns)
                        continue;  // (types 4 and 6 have no key)
                    for (int format : {ZS_PNG_FMT_RGBA8, ZS_PNG_FMT_RGBA16})
                        for (int residue = 0; residue < 16; residue += png_expand_bytes(format))
                            if (!run_case(im, format, residue)) return 1;
                }
    // every table entry, as the rules give it
    for (int entries : kEntries) {
        std::vector<uint8_t> plte((size_t)entries * 3), trns((size_t)(entries + 1) / 2);
        for (auto &b : plte) b = (uint8_t)rng();
        for (auto &b : trns) b = (uint8_t)rng();
        uint32_t table[kPngPalEntries];
        png_expand_table(plte.data(), entries, trns.data(), (int)trns.size(), table);
        for (int k = 0; k < kPngPalEntries; k++) {
            const uint32_t want = k >= entries ? 0xFF000000u
                                               : (uint32_t)plte[3 * (size_t)k] + 256u * plte[3 * (size_t)k + 1] + 65536u * plte[3 * (size_t)k + 2] +
                                                     16777216u * (k < (int)trns.size() ? trns[(size_t)k] : 255u);
            if (table[k] != want) return printf("FAIL table of %d entries: entry %d is %08x, expected %08x\n", entries, k, table[k], want), 1;
        }
    }
    if (png_expand_bytes(ZS_PNG_FMT_RGBA8) != 4 || png_expand_bytes(ZS_PNG_FMT_RGBA16) != 8) return printf("FAIL png_expand_bytes\n"), 1;
    if (g_keyed == 0 || g_beyond == 0) return printf("FAIL the cases hold no keyed pixel or no index beyond a palette (%ld, %ld)\n", g_keyed, g_beyond), 1;
    printf("PASS %ld cases, %ld keyed pixels, %ld indexes beyond their palette\n", g_cases, g_keyed, g_beyond);
    return 0;
}
