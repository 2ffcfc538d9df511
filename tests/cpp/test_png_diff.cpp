// test_png_diff.cpp -- the frame diff (zlibstream_amd/csrc/zs_png.hip, KD), the crop and the closing of a chunk with a
// prefix (zs_crc32.hip's finishing launch) run on the host with the code the kernels compile: zs_png.h png_diff_load,
// png_diff_group, png_diff_record, png_diff_merge / png_diff_union / png_diff_finish, png_crop_group, and zs_crc32.h
// png_close_chunk.  The diff is driven the way the device drives it: a row cut into stretches of 64 groups, a "wave" of 64
// lanes per stretch, each lane carrying its group from canvas to canvas, the ballot modelled with a 64-bit mask, one record
// per wave and frame, the records folded in an order that differs from the device's.  Compared with a restatement written
// here, pixel by pixel: the smallest rectangle that holds every pixel whose bytes differ.  The canvases lie in a buffer that is
// exactly as long as they are (a read outside shows under -fsanitize=address); the crop's outputs start poisoned and have
// guard bytes on both sides.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_crc32.h"
#include "../../zlibstream_amd/csrc/zs_png.h"

using namespace zs;

namespace {

struct Rect {
    int64_t x, y, w, h;
};
bool same(const Rect &a, const Rect &b) { return a.x == b.x && a.y == b.y && a.w == b.w && a.h == b.h; }

long g_diffs = 0, g_wide_loads = 0, g_narrow_loads = 0, g_crops = 0, g_crop_wide = 0, g_crop_mixed = 0;

// ---- the rule, restated: frame 0 is the canvas; frame f the bounding box of the differing pixels, 1 x 1 at (0, 0) if none
std::vector<Rect> restate(const uint8_t *cv, int w, int h, int nf, int P) {
    std::vector<Rect> out{Rect{0, 0, w, h}};
    const size_t canvas = (size_t)w * h * P;
    for (int f = 1; f < nf; f++) {
        int x0 = w, y0 = h, x1 = -1, y1 = -1;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                if (memcmp(cv + (size_t)f * canvas + ((size_t)y * w + x) * P, cv + (size_t)(f - 1) * canvas + ((size_t)y * w + x) * P, (size_t)P) != 0) {
                    if (x < x0) x0 = x;
                    if (x > x1) x1 = x;
                    if (y < y0) y0 = y;
                    if (y > y1) y1 = y;
                }
        out.push_back(x1 < 0 ? Rect{0, 0, 1, 1} : Rect{x0, y0, x1 - x0 + 1, y1 - y0 + 1});
    }
    return out;
}

// ---- the device's way: waves of 64 lanes over the stretches of every row
template <int F>
std::vector<Rect> model(const uint8_t *cv, int w, int h, int nf) {
    constexpr int P = png_expand_bytes(F), N = kPngComposeGroup / P;
    const int64_t per_row = png_compose_row_waves(w, F), waves = per_row * h, rb = (int64_t)w * P, canvas = rb * h;
    std::vector<PngDiffRec> recs((size_t)(waves * (nf - 1)), PngDiffRec{123, 456});  // (every slot must be written)
    for (int64_t t = waves - 1; t >= 0; t--) {  // (waves in any order: none depends on another)
        const int64_t y = t / per_row, g0 = (t % per_row) * 64;
        uint64_t prev[64][2];
        for (int lane = 0; lane < 64; lane++) {
            const int64_t x0 = (g0 + lane) * N;
            prev[lane][0] = prev[lane][1] = 0;
            if (x0 < w) png_diff_load<F>(cv + y * rb + x0 * P, x0, w, prev[lane]);
        }
        for (int f = 1; f < nf; f++) {
            uint64_t mask = 0;
            int first[64], last[64];
            for (int lane = 0; lane < 64; lane++) {
                const int64_t x0 = (g0 + lane) * N;
                first[lane] = last[lane] = 0;
                if (x0 >= w) continue;
                const uint8_t *p = cv + (int64_t)f * canvas + y * rb + x0 * P;
                uint64_t cur[2];
                png_diff_load<F>(p, x0, w, cur);
                if (x0 + N <= w && ((uintptr_t)p & 15) == 0) g_wide_loads++;
                else g_narrow_loads++;
                if (png_diff_group<F>(prev[lane], cur, &first[lane], &last[lane])) mask |= 1ull << lane;
                prev[lane][0] = cur[0], prev[lane][1] = cur[1];
            }
            PngDiffRec rec = png_diff_none();
            if (mask) {
                const int lo = png_diff_first_lane(mask), hi = png_diff_last_lane(mask);
                rec = png_diff_record(lo, hi, g0, N, first[lo], last[hi]);
            }
            recs[(size_t)((f - 1) * waves + t)] = rec;
        }
    }
    std::vector<Rect> out{Rect{0, 0, w, h}};
    for (int f = 1; f < nf; f++) {
        // four partial rectangles over interleaved records, then their union: not the order of the device's lanes
        PngDiffRect part[4] = {png_diff_empty(), png_diff_empty(), png_diff_empty(), png_diff_empty()};
        for (int64_t k = waves - 1; k >= 0; k--) part[k & 3] = png_diff_merge(part[k & 3], recs[(size_t)((f - 1) * waves + k)], (int32_t)(k / per_row));
        const PngDiffRect r = png_diff_union(png_diff_union(part[3], part[1]), png_diff_union(part[0], part[2]));
        Rect q;
        png_diff_finish(r, &q.x, &q.y, &q.w, &q.h);
        out.push_back(q);
    }
    return out;
}

// one change of a canvas against the one before it
struct Change {
    int x, y;
    int kind;  // 0: every byte of the pixel; 1: the alpha's bytes only; 2: the low byte of one sample only; 3: a colour byte (the caller made alpha 0)
};

void apply(std::vector<uint8_t> &c, int w, int P, const Change &ch, int salt) {
    uint8_t *p = c.data() + ((size_t)ch.y * w + ch.x) * P;
    if (ch.kind == 0)
        for (int b = 0; b < P; b++) p[b] ^= (uint8_t)(0x11 * (b + 1) + salt) | 1;
    else if (ch.kind == 1) p[P - 1] ^= 0x40;                // alpha (RGBA16: its high byte)
    else if (ch.kind == 2) p[P == 8 ? 2 : 1] ^= 0x01;       // G (RGBA16: little-endian, so byte 2 is G's low byte)
    else p[0] ^= 0x80;                                       // R, under alpha 0
}

bool run_case(int format, int w, int h, const std::vector<std::vector<Change>> &steps, int residue, const char *what, std::mt19937_64 &rng, bool back_to_first = false) {
    const int P = png_expand_bytes(format), nf = (int)steps.size() + 1;
    const size_t canvas = (size_t)w * h * P;
    std::vector<uint8_t> first(canvas);
    for (auto &b : first) b = (uint8_t)rng();
    for (const auto &st : steps)
        for (const Change &ch : st)
            if (ch.kind == 3) memset(first.data() + ((size_t)ch.y * w + ch.x) * P + (P - P / 4), 0, (size_t)P / 4);  // alpha 0 from canvas 0 on
    std::vector<std::vector<uint8_t>> cvs{first};
    for (size_t k = 0; k < steps.size(); k++) {
        std::vector<uint8_t> c = cvs.back();
        for (const Change &ch : steps[k]) apply(c, w, P, ch, (int)k);
        if (back_to_first && k == 1) c = first;  // A, B, A
        cvs.push_back(c);
    }
    // the canvases back to back at the residue asked for, the last one ending where the buffer ends
    std::vector<uint8_t> buf(canvas * nf + 16);
    const size_t lead = ((size_t)residue + 16 - (uintptr_t)buf.data() % 16) % 16;
    buf.resize(lead + canvas * nf);  // (shrinks: the storage stays where it is)
    uint8_t *base = buf.data() + lead;
    if ((uintptr_t)base % 16 != (uintptr_t)residue) return printf("FAIL set-up: residue %d not reached\n", residue), false;
    for (int f = 0; f < nf; f++) memcpy(base + (size_t)f * canvas, cvs[(size_t)f].data(), canvas);
    const std::vector<Rect> want = restate(base, w, h, nf, P);
    const std::vector<Rect> got = format == ZS_PNG_FMT_RGBA8 ? model<ZS_PNG_FMT_RGBA8>(base, w, h, nf) : model<ZS_PNG_FMT_RGBA16>(base, w, h, nf);
    for (int f = 0; f < nf; f++)
        if (!same(want[(size_t)f], got[(size_t)f])) {
            printf("FAIL %s: %dx%d format %d, %d frames, residue %d, frame %d: got %lld,%lld %lldx%lld, want %lld,%lld %lldx%lld\n", what, w, h, format, nf, residue, f,
                   (long long)got[(size_t)f].x, (long long)got[(size_t)f].y, (long long)got[(size_t)f].w, (long long)got[(size_t)f].h, (long long)want[(size_t)f].x,
                   (long long)want[(size_t)f].y, (long long)want[(size_t)f].w, (long long)want[(size_t)f].h);
            return false;
        }
    g_diffs++;
    return true;
}

bool test_group() {
    // every single byte, and every pair of bytes, of a group
    for (int format = 0; format < 2; format++) {
        const int P = png_expand_bytes(format);
        for (int i = 0; i < 16; i++)
            for (int j = i; j < 16; j++) {
                uint8_t a[16], b[16];
                for (int k = 0; k < 16; k++) a[k] = b[k] = (uint8_t)(17 * k + 3);
                b[i] ^= 0x01, b[j] ^= 0x80;
                uint64_t va[2], vb[2];
                memcpy(va, a, 16), memcpy(vb, b, 16);
                int first = -1, last = -1;
                const bool d = format == 0 ? png_diff_group<ZS_PNG_FMT_RGBA8>(va, vb, &first, &last) : png_diff_group<ZS_PNG_FMT_RGBA16>(va, vb, &first, &last);
                if (!d || first != i / P || last != j / P) return printf("FAIL group format %d bytes %d, %d: %d, first %d, last %d\n", format, i, j, (int)d, first, last), false;
                int f2 = -7, l2 = -7;
                const bool e = format == 0 ? png_diff_group<ZS_PNG_FMT_RGBA8>(va, va, &f2, &l2) : png_diff_group<ZS_PNG_FMT_RGBA16>(va, va, &f2, &l2);
                if (e) return printf("FAIL group: equal groups differ\n"), false;
            }
    }
    for (int lo = 0; lo < 64; lo++)
        for (int hi = lo; hi < 64; hi++) {
            const uint64_t m = 1ull << lo | 1ull << hi | (hi - lo > 1 ? 1ull << (lo + 1) : 0);
            if (png_diff_first_lane(m) != lo || png_diff_last_lane(m) != hi) return printf("FAIL lanes %d, %d\n", lo, hi), false;
        }
    return true;
}

bool test_diff() {
    std::mt19937_64 rng(991);
    struct Shape {
        int w, h;
    };
    const Shape shapes[] = {{1, 1}, {1, 5}, {3, 1}, {5, 3}, {261, 2}, {257, 3}, {129, 3}};
    for (int format = 0; format < 2; format++) {
        const int P = png_expand_bytes(format), N = 16 / P;
        for (const Shape &s : shapes) {
            const int w = s.w, h = s.h;
            // the single changes: corners, edges, both sides of a group's and of a stretch's boundary, the three partial kinds
            std::vector<std::vector<Change>> singles;
            singles.push_back({});  // no change
            for (int cy : {0, h - 1})
                for (int cx : {0, w - 1}) singles.push_back({Change{cx, cy, 0}});
            singles.push_back({Change{w / 2, 0, 0}}), singles.push_back({Change{w / 2, h - 1, 0}}), singles.push_back({Change{0, h / 2, 0}}), singles.push_back({Change{w - 1, h / 2, 0}});
            for (int cx : {N - 1, N, 64 * N - 1, 64 * N})
                if (cx < w) singles.push_back({Change{cx, h / 2, 0}}), singles.push_back({Change{cx, h - 1, 1}});
            singles.push_back({Change{w / 2, h / 2, 1}}), singles.push_back({Change{w / 3, h / 2, 2}}), singles.push_back({Change{w - 1, 0, 3}});
            singles.push_back({Change{0, 0, 0}, Change{w - 1, h - 1, 0}}), singles.push_back({Change{w - 1, 0, 0}, Change{0, h - 1, 0}});  // opposite corners
            for (int residue = 0; residue < 16; residue += P) {
                if (!run_case(format, w, h, {}, residue, "one frame", rng)) return false;
                for (size_t k = 0; k < singles.size(); k++) {
                    if (!run_case(format, w, h, {singles[k]}, residue, "two frames", rng)) return false;
                    // three frames: the second change alone is frame 2 -- a diff against canvas 0 would hold both
                    if (!run_case(format, w, h, {singles[k], singles[(k + 5) % singles.size()]}, residue, "three frames", rng)) return false;
                }
                // A, B, A: frame 2 is B's change again, not "nothing"
                for (size_t k = 1; k < singles.size(); k += 3)
                    if (!run_case(format, w, h, {singles[k], {}}, residue, "A, B, A", rng, true)) return false;
                // nine frames: the changes in turn
                for (size_t k = 0; k < singles.size(); k += 4) {
                    std::vector<std::vector<Change>> steps;
                    for (size_t j = 0; j < 8; j++) steps.push_back(singles[(k + 3 * j) % singles.size()]);
                    if (!run_case(format, w, h, steps, residue, "nine frames", rng)) return false;
                }
            }
        }
    }
    return true;
}

// ---- the crop
template <int P>
void crop_model(const PngCropImg &im) {
    const int64_t rb = (int64_t)im.width * P;
    for (int64_t y = im.height - 1; y >= 0; y--) {
        uint8_t *dst = im.out + y * rb;
        const uint64_t addr = (uint64_t)(uintptr_t)dst;
        const int64_t ng = adam7_row_groups(addr, rb, 16), b0 = adam7_row_b0(addr, 16);
        for (int64_t g = ng - 1; g >= 0; g--) {
            png_crop_group<P>(im, y, rb, dst, b0 + g * 16);
            const int64_t at = b0 + g * 16;
            if (at >= 0 && at + 16 <= rb) (((uintptr_t)(im.in + y * im.in_pitch + at) & 15) == 0 ? g_crop_wide : g_crop_mixed)++;
        }
    }
}

bool test_crop() {
    std::mt19937_64 rng(4242);
    constexpr int kGuard = 48;
    for (int P : {4, 8}) {
        const int iw = 23, ih = 7;
        const Rect rects[] = {{0, 0, iw, ih}, {0, 0, 1, 1}, {iw - 1, ih - 1, 1, 1}, {0, 2, 9, 3}, {14, 0, 9, 2}, {3, 4, 17, 3}, {5, 1, 1, 5}, {iw - 1, 0, 1, ih}, {2, 2, 13, 1}, {1, 1, 21, 5}};
        for (int sres = 0; sres < 16; sres += P)
            for (int dres = 0; dres < 16; dres += P)
                for (const Rect &r : rects) {
                    std::vector<uint8_t> img((size_t)iw * ih * P + 32);
                    uint8_t *in = img.data() + (16 - (uintptr_t)img.data() % 16) % 16 + sres;
                    for (size_t k = 0; k < (size_t)iw * ih * P; k++) in[k] = (uint8_t)rng();
                    const size_t total = (size_t)(r.w * r.h * P);
                    std::vector<uint8_t> buf(total + 2 * kGuard + 32, 0xA5);
                    uint8_t *out = buf.data() + kGuard;
                    out += (16 - (uintptr_t)out % 16) % 16 + dres;
                    const PngCropImg im{in + (r.y * iw + r.x) * P, out, (int64_t)iw * P, (int32_t)r.w, (int32_t)r.h};
                    if (P == 4) crop_model<4>(im);
                    else crop_model<8>(im);
                    for (uint8_t *p = buf.data(); p < buf.data() + buf.size(); p++)
                        if ((p < out || p >= out + total) && *p != 0xA5) return printf("FAIL crop guard: P %d, residues %d -> %d\n", P, sres, dres), false;
                    for (int64_t y = 0; y < r.h; y++)
                        for (int64_t x = 0; x < r.w; x++)
                            if (memcmp(out + (y * r.w + x) * P, in + ((r.y + y) * iw + r.x + x) * P, (size_t)P) != 0)
                                return printf("FAIL crop: P %d, residues %d -> %d, %lld,%lld %lldx%lld, pixel (%lld, %lld)\n", P, sres, dres, (long long)r.x, (long long)r.y,
                                              (long long)r.w, (long long)r.h, (long long)x, (long long)y),
                                       false;
                    g_crops++;
                }
    }
    return true;
}

// ---- the closing of a chunk.  The expected bytes are png_anim_ref.chunk(b"IDAT", data) and png_anim_ref.fdat(seq, data) of
// tests/png_anim_ref.py (struct.pack and zlib.crc32), written out.
bool close_case(const char *type4, bool has_prefix, uint32_t prefix, const std::vector<uint8_t> &data, const std::vector<uint8_t> &want) {
    const size_t head = has_prefix ? 12 : 8;
    std::vector<uint8_t> buf(head + data.size() + 4 + 16, 0xA5);
    uint8_t *f = buf.data() + 8;  // (guard bytes on both sides)
    if (want.size() != head + data.size() + 4) return printf("FAIL close: the expectation has the wrong length\n"), false;
    if (!data.empty()) memcpy(f + head, data.data(), data.size());
    // the host's seed -- the register behind the type and the prefix -- and the data fed behind it, as the device does
    uint8_t tp[8];
    memcpy(tp, type4, 4);
    png_put_be32(tp + 4, prefix);
    const uint32_t init = ~crc32_bytes_slow(0, tp, has_prefix ? 8 : 4);
    const uint32_t crc = crc32_bytes_slow(~init, data.data(), data.size());
    png_close_chunk(f, (uint32_t)data.size(), png_type(type4[0], type4[1], type4[2], type4[3]), has_prefix, prefix, crc);
    if (memcmp(f, want.data(), want.size()) != 0) return printf("FAIL close %s prefix %d: bytes differ\n", type4, (int)has_prefix), false;
    for (size_t k = 0; k < buf.size(); k++)
        if ((k < 8 || k >= 8 + want.size()) && buf[k] != 0xA5) return printf("FAIL close %s: a byte outside the chunk was written\n", type4), false;
    return true;
}

bool test_close() {
    const std::vector<uint8_t> hello = {'h', 'e', 'l', 'l', 'o'};
    std::vector<uint8_t> forty(40);
    for (int k = 0; k < 40; k++) forty[(size_t)k] = (uint8_t)k;
    std::vector<uint8_t> want_forty = {0x00, 0x00, 0x00, 0x2C, 0x66, 0x64, 0x41, 0x54, 0x00, 0x01, 0x00, 0x00};
    want_forty.insert(want_forty.end(), forty.begin(), forty.end());
    for (uint8_t b : {0xB9, 0x5F, 0xF4, 0x48}) want_forty.push_back(b);
    return close_case("IDAT", false, 0, hello, {0x00, 0x00, 0x00, 0x05, 0x49, 0x44, 0x41, 0x54, 0x68, 0x65, 0x6C, 0x6C, 0x6F, 0xBC, 0xBE, 0x08, 0x52}) &&
           close_case("fdAT", true, 7, hello, {0x00, 0x00, 0x00, 0x09, 0x66, 0x64, 0x41, 0x54, 0x00, 0x00, 0x00, 0x07, 0x68, 0x65, 0x6C, 0x6C, 0x6F, 0xC0, 0x38, 0x95, 0x48}) &&
           close_case("IDAT", false, 0, {}, {0x00, 0x00, 0x00, 0x00, 0x49, 0x44, 0x41, 0x54, 0x35, 0xAF, 0x06, 0x1E}) &&
           close_case("fdAT", true, 0x01020304u, {}, {0x00, 0x00, 0x00, 0x04, 0x66, 0x64, 0x41, 0x54, 0x01, 0x02, 0x03, 0x04, 0x92, 0xB0, 0x8A, 0xB0}) &&
           close_case("fdAT", true, 65536, forty, want_forty);
}

}  // namespace

int main() {
    if (!test_group() || !test_diff() || !test_crop() || !test_close()) return 1;
    if (g_wide_loads == 0 || g_narrow_loads == 0 || g_crop_wide == 0 || g_crop_mixed == 0)
        return printf("FAIL coverage: %ld / %ld wide / narrow loads, %ld / %ld crop groups with / without a 16-byte load\n", g_wide_loads, g_narrow_loads, g_crop_wide, g_crop_mixed), 1;
    printf("PASS %ld animations diffed (%ld 16-byte loads, %ld by pixels), %ld crops\n", g_diffs, g_wide_loads, g_narrow_loads, g_crops);
    return 0;
}
