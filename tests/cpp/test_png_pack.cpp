// test_png_pack.cpp -- the pack of RGBA8 / RGBA16 pixels into raw PNG scanlines (zlibstream_amd/csrc/zs_png.hip, KG) run on the
// host with the code the kernel compiles (zs_png.h png_pack_group): whole rows, group by group as a wave's lanes take them, at
// all fifteen (colour type, bit depth) pairs, both formats, with the output row at every residue modulo 16.  Compared with a
// per-pixel restatement of the rules written here: divisions where the header shifts, the palette searched entry by entry
// where the header probes a hash table, samples put into the row bit by bit.
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
    int w, h, ct, d, format;
    std::vector<uint8_t> px;  // h rows of w * 4 bytes or w * 4 uint16
    std::vector<uint8_t> plte, trns;
};

uint32_t source(const Image &im, int x, int y, int k) {
    const size_t at = ((size_t)y * im.w + x) * 4 + k;
    if (im.format == ZS_PNG_FMT_RGBA8) return im.px[at];
    uint16_t v;
    memcpy(&v, im.px.data() + 2 * at, 2);
    return v;
}
void put_source(Image &im, int x, int y, int k, uint32_t v) {
    const size_t at = ((size_t)y * im.w + x) * 4 + k;
    if (im.format == ZS_PNG_FMT_RGBA8) im.px[at] = (uint8_t)v;
    else {
        const uint16_t s = (uint16_t)v;
        memcpy(im.px.data() + 2 * at, &s, 2);
    }
}

// The rules, per sample: from a source of 8 or 16 bits to depth d.
uint32_t reduce(uint32_t v, int format, int d) {
    if (format == ZS_PNG_FMT_RGBA8) return d == 16 ? v * 257 : v / (256u >> d);
    if (d == 16) return v;
    return ((v * 255 + 32895) / 65536) / (256u >> d);
}

// sample k of pixel x into a row of the file's layout, bit by bit from the top
void put_bits(uint8_t *row, int64_t bit0, int d, uint32_t v) {
    for (int j = 0; j < d; j++) {
        const int64_t bit = bit0 + j;
        if ((v >> (d - 1 - j)) & 1) row[bit / 8] |= (uint8_t)(0x80 >> (bit % 8));
    }
}

long g_cases = 0, g_keyed = 0, g_missed = 0, g_dups = 0;

// the expected rows and the expected count of palette pixels without an entry
void restate(const Image &im, std::vector<uint8_t> &want, int64_t *misses) {
    const int ch = channels(im.ct);
    const int64_t rb = ((int64_t)im.w * im.d * ch + 7) / 8;
    want.assign((size_t)(rb * im.h), 0);
    *misses = 0;
    for (int y = 0; y < im.h; y++)
        for (int x = 0; x < im.w; x++) {
            uint32_t s[4] = {0, 0, 0, 0};
            if (im.ct == 3) {
                uint32_t c[4];
                for (int k = 0; k < 4; k++) c[k] = reduce(source(im, x, y, k), im.format, 8);
                int found = -1;
                for (int e = 0; e < (int)im.plte.size() / 3 && found < 0; e++) {
                    const uint32_t a = e < (int)im.trns.size() ? im.trns[(size_t)e] : 255;
                    if (im.plte[3 * (size_t)e] == c[0] && im.plte[3 * (size_t)e + 1] == c[1] && im.plte[3 * (size_t)e + 2] == c[2] && a == c[3]) found = e;
                }
                if (found < 0) ++*misses, found = 0;
                s[0] = (uint32_t)found;
            } else if (im.ct == 0 || im.ct == 2) {
                const bool keyed = !im.trns.empty() && source(im, x, y, 3) == 0;
                for (int k = 0; k < ch; k++)
                    s[k] = keyed ? ((uint32_t)im.trns[2 * (size_t)k] * 256 + im.trns[2 * (size_t)k + 1]) % (1u << im.d) : reduce(source(im, x, y, k), im.format, im.d);
                if (keyed) g_keyed++;
            } else if (im.ct == 4) {
                s[0] = reduce(source(im, x, y, 0), im.format, im.d), s[1] = reduce(source(im, x, y, 3), im.format, im.d);
            } else
                for (int k = 0; k < 4; k++) s[k] = reduce(source(im, x, y, k), im.format, im.d);
            for (int k = 0; k < ch; k++) put_bits(want.data() + y * rb, ((int64_t)x * ch + k) * im.d, im.d, s[k]);
        }
}

bool run_case(const Image &im, const std::vector<uint8_t> &want, int64_t want_miss, int residue) {
    const int bits = im.d * channels(im.ct);
    const int64_t rb = png_bits_row_bytes(im.w, bits), total = rb * im.h;
    constexpr int kGuard = 64;
    std::vector<uint8_t> buf((size_t)(total + 2 * kGuard + 32), 0xA5);
    uint8_t *base = buf.data() + kGuard;
    base += (16 - (uintptr_t)base % 16) % 16 + residue;  // the first row's residue; the others follow from the row length

    std::vector<uint32_t> tables(3 * kPngPackTableWords, 0x12345678u);  // the image's table is the second of three
    PngPackImg d{im.px.data(), base, im.w, im.h, im.d, im.ct, im.format, 0, {0, 0, 0}, 0};
    if (im.ct == 3) {
        d.pal_off = kPngPackTableWords;
        png_pack_table(im.plte.data(), (int)im.plte.size() / 3, im.trns.data(), (int)im.trns.size(), tables.data() + d.pal_off);
    } else if (!im.trns.empty()) {
        for (int j = 0; j < (im.ct == 0 ? 1 : 3); j++) d.key[j] = (uint16_t)(im.trns[2 * (size_t)j] * 256 + im.trns[2 * (size_t)j + 1]);
        d.has_key = 1;
    }
    const int G = png_pack_group_bytes(bits);
    int64_t miss = 0;
    for (int y = 0; y < im.h; y++) {
        uint8_t *dst = base + y * rb;
        const uint64_t addr = (uint64_t)(uintptr_t)dst;
        const int64_t ng = adam7_row_groups(addr, rb, G), b0 = adam7_row_b0(addr, G);
        // (the lanes of a wave in any order: no group depends on another)
        for (int64_t g = ng - 1; g >= 0; g--) {
            if (im.format == ZS_PNG_FMT_RGBA8) miss += png_pack_group<ZS_PNG_FMT_RGBA8>(d, tables.data() + d.pal_off, y, rb, dst, b0 + g * G);
            else miss += png_pack_group<ZS_PNG_FMT_RGBA16>(d, tables.data() + d.pal_off, y, rb, dst, b0 + g * G);
        }
    }
    for (uint8_t *p = buf.data(); p < buf.data() + buf.size(); p++)
        if ((p < base || p >= base + total) && *p != 0xA5) {
            printf("FAIL guard: type %d depth %d format %d %dx%d residue %d: byte %td of the buffer (row data is %td .. %td)\n", im.ct, im.d, im.format, im.w,
                   im.h, residue, p - buf.data(), base - buf.data(), base + total - buf.data());
            return false;
        }
    for (int64_t k = 0; k < total; k++)
        if (base[k] != want[(size_t)k]) {
            printf("FAIL type %d depth %d format %d %dx%d residue %d trns %zu plte %zu: byte %lld of row %lld is %02x, expected %02x\n", im.ct, im.d, im.format,
                   im.w, im.h, residue, im.trns.size(), im.plte.size() / 3, (long long)(k % rb), (long long)(k / rb), base[k], want[(size_t)k]);
            return false;
        }
    if (miss != want_miss) {
        printf("FAIL type %d depth %d format %d %dx%d residue %d: %lld pixels without an entry, expected %lld\n", im.ct, im.d, im.format, im.w, im.h, residue,
               (long long)miss, (long long)want_miss);
        return false;
    }
    g_cases++;
    return true;
}

}  // namespace

int main() {
    std::mt19937 rng(20240911);
    std::vector<int> widths;
    for (int w = 1; w <= 70; w++) widths.push_back(w);
    for (int w : {255, 256, 257, 513}) widths.push_back(w);
    const int kEntries[5] = {1, 2, 16, 255, 256};
    int pal_turn = 0;
    for (const auto &pair : kPairs)
        for (int w : widths)
            for (int h : {1, 3})
                for (int with_trns = 0; with_trns < 2; with_trns++)
                    for (int format : {ZS_PNG_FMT_RGBA8, ZS_PNG_FMT_RGBA16}) {
                        Image im{w, h, pair[0], pair[1], format, {}, {}, {}};
                        const uint32_t top = format == ZS_PNG_FMT_RGBA8 ? 255 : 65535;
                        im.px.resize((size_t)w * h * png_expand_bytes(format));
                        for (auto &b : im.px) b = (uint8_t)rng();
                        if (im.ct == 3) {
                            // a palette with the entry 0,0,0,0 and duplicates (of colour and alpha: only the first can be named)
                            const int entries = std::min(kEntries[pal_turn++ % 5], 1 << im.d);
                            im.plte.resize((size_t)entries * 3);
                            for (auto &b : im.plte) b = (uint8_t)rng();
                            if (with_trns) {
                                im.trns.resize((size_t)(1 + rng() % (unsigned)entries));
                                for (auto &b : im.trns) b = (uint8_t)rng();
                                const int z = (int)(rng() % (unsigned)im.trns.size());
                                im.plte[3 * (size_t)z] = im.plte[3 * (size_t)z + 1] = im.plte[3 * (size_t)z + 2] = 0, im.trns[(size_t)z] = 0;
                            }
                            if (entries >= 2) {
                                const int from = (int)(rng() % (unsigned)(entries - 1)), to = from + 1 + (int)(rng() % (unsigned)(entries - 1 - from));
                                memcpy(&im.plte[3 * (size_t)to], &im.plte[3 * (size_t)from], 3);
                                if (to < (int)im.trns.size()) im.trns[(size_t)to] = im.trns[(size_t)from];
                                else if (from < (int)im.trns.size()) im.trns[(size_t)from] = 255;
                                g_dups++;
                            }
                            // the pixels: entries of the palette, a few of them one bit off (no entry, unless another one happens to match)
                            for (int y = 0; y < h; y++)
                                for (int x = 0; x < w; x++) {
                                    const int e = (int)(rng() % (unsigned)entries);
                                    uint32_t c[4] = {im.plte[3 * (size_t)e], im.plte[3 * (size_t)e + 1], im.plte[3 * (size_t)e + 2],
                                                     e < (int)im.trns.size() ? im.trns[(size_t)e] : 255u};
                                    if (rng() % 7 == 0) c[rng() % 4] ^= 1u << (rng() % 8);
                                    for (int k = 0; k < 4; k++) put_source(im, x, y, k, format == ZS_PNG_FMT_RGBA8 ? c[k] : c[k] * 257);
                                }
                        } else if (with_trns && (im.ct == 0 || im.ct == 2)) {
                            // a key with bits above the depth set in the chunk (they do not count); alpha 0 on some pixels, 1 and the
                            // maximum on others (not keyed)
                            im.trns.resize(im.ct == 0 ? 2 : 6);
                            for (auto &b : im.trns) b = (uint8_t)rng();
                            for (int y = 0; y < h; y++)
                                for (int x = 0; x < w; x++) {
                                    const unsigned t = rng() % 4;
                                    if (t < 3) put_source(im, x, y, 3, t == 0 ? 0 : t == 1 ? 1 : top);
                                }
                        } else if (with_trns)
                            continue;  // (types 4 and 6 have no key)
                        std::vector<uint8_t> want;
                        int64_t want_miss;
                        restate(im, want, &want_miss);
                        g_missed += want_miss;
                        for (int residue = 0; residue < 16; residue++)
                            if (!run_case(im, want, want_miss, residue)) return 1;
                    }
    // every table: each entry is found at the first index of its colour, and a colour that is in no entry is not found
    for (int entries : kEntries)
        for (int round = 0; round < 20; round++) {
            std::vector<uint8_t> plte((size_t)entries * 3), trns((size_t)(entries + 1) / 2);
            for (auto &b : plte) b = (uint8_t)(rng() % (round < 10 ? 256 : 3));  // (few values: many duplicates)
            for (auto &b : trns) b = (uint8_t)(rng() % (round < 10 ? 256 : 2));
            if (round % 2) plte[0] = plte[1] = plte[2] = 0, trns[0] = 0;
            uint32_t table[kPngPackTableWords];
            png_pack_table(plte.data(), entries, trns.data(), (int)trns.size(), table);
            auto color = [&](int k) {
                return (uint32_t)plte[3 * (size_t)k] + 256u * plte[3 * (size_t)k + 1] + 65536u * plte[3 * (size_t)k + 2] + 16777216u * (k < (int)trns.size() ? trns[(size_t)k] : 255u);
            };
            for (int k = 0; k < entries; k++) {
                int first = 0;
                while (color(first) != color(k)) first++;
                if (png_pack_lookup(table, color(k)) != first)
                    return printf("FAIL table of %d entries: entry %d (%08x) is found at %d, expected %d\n", entries, k, color(k), png_pack_lookup(table, color(k)), first), 1;
            }
            for (int t = 0; t < 2000; t++) {
                const uint32_t c = t == 0 ? 0u : t == 1 ? 0xFFFFFFFFu : (uint32_t)rng();
                int first = -1;
                for (int k = 0; k < entries && first < 0; k++)
                    if (color(k) == c) first = k;
                if (png_pack_lookup(table, c) != first) return printf("FAIL table of %d entries: colour %08x is found at %d, expected %d\n", entries, c, png_pack_lookup(table, c), first), 1;
            }
        }
    // the choice, on the points the rule names
    struct Choice {
        bool opaque, gray, low8;
        int depth, colors, ct, bd;
    };
    const Choice kChoices[] = {{true, true, true, 1, 2, 0, 1},    {true, true, true, 8, 200, 0, 8},   {true, true, true, 8, 3, 3, 2},     {true, true, true, 4, 3, 3, 2},
                               {true, true, true, 2, 3, 0, 2},    {true, true, true, 4, 16, 0, 4},    {true, true, true, 8, 16, 3, 4},    {true, true, true, 8, 2, 3, 1},
                               {false, true, true, 8, 257, 4, 8}, {false, true, true, 1, 256, 3, 8},  {true, false, true, 8, 257, 2, 8},  {true, false, true, 8, 256, 3, 8},
                               {false, false, true, 8, 257, 6, 8}, {false, false, true, 8, 17, 3, 8}, {true, true, false, 16, 257, 0, 16}, {false, true, false, 16, 257, 4, 16},
                               {true, false, false, 16, 257, 2, 16}, {false, false, false, 16, 257, 6, 16}};
    for (const Choice &k : kChoices) {
        int ct = -1, bd = -1;
        png_choose_format(k.opaque, k.gray, k.low8, k.depth, k.colors, &ct, &bd);
        if (ct != k.ct || bd != k.bd)
            return printf("FAIL choice: opaque %d gray %d low8 %d depth %d colours %d gives (%d, %d), expected (%d, %d)\n", k.opaque, k.gray, k.low8, k.depth, k.colors,
                          ct, bd, k.ct, k.bd), 1;
    }
    if (g_keyed == 0 || g_missed == 0 || g_dups == 0) return printf("FAIL the cases hold no keyed pixel, no pixel without an entry or no duplicate (%ld, %ld, %ld)\n", g_keyed, g_missed, g_dups), 1;
    printf("PASS %ld cases, %ld keyed pixels, %ld pixels without an entry\n", g_cases, g_keyed, g_missed);
    return 0;
}
