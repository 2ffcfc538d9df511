// test_png_compose.cpp -- the composing of an animated PNG's frames into canvases (zlibstream_amd/csrc/zs_png.hip, KM) run on
// the host with the code the kernel compiles (zs_png.h png_blend_over, png_compose_dispose, png_compose_group): whole rows,
// group by group as a wave's lanes take them.  Compared with a restatement written here from the APNG specification: the
// blend channel by channel on arrays, the animation frame by frame on a full canvas that is copied out after every frame
// and patched by the dispose operation -- where the header carries each pixel through all frames on its own.
// The frame buffers are exactly as long as their regions (a read outside shows under -fsanitize=address); the output starts
// poisoned and has guard bytes on both sides: a byte not written, or written outside, shows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_png.h"

using namespace zs;

namespace {

struct Px {
    uint32_t c[4];  // R, G, B, A
};
bool same(const Px &a, const Px &b) { return memcmp(a.c, b.c, sizeof a.c) == 0; }

// ---- the rules, restated ----
// APNG specification, "blend_op": APNG_BLEND_OP_OVER composites as in the PNG specification's "Alpha Channel Processing"
// sample code, here with integers: M is the maximum sample.
Px over(const Px &fg, const Px &bg, uint64_t M) {
    if (fg.c[3] == 0) return bg;
    if (fg.c[3] == M || bg.c[3] == 0) return fg;
    const uint64_t u = (uint64_t)fg.c[3] * M, v = (M - fg.c[3]) * (uint64_t)bg.c[3], al = u + v;
    Px r;
    for (int k = 0; k < 3; k++) r.c[k] = (uint32_t)((unsigned __int128)((unsigned __int128)fg.c[k] * u + (unsigned __int128)bg.c[k] * v) / al);
    r.c[3] = (uint32_t)(al / M);
    return r;
}

uint64_t pack(const Px &p, int format) {
    if (format == ZS_PNG_FMT_RGBA8) return (uint64_t)(p.c[0] | p.c[1] << 8 | p.c[2] << 16 | p.c[3] << 24);
    return (uint64_t)p.c[0] | (uint64_t)p.c[1] << 16 | (uint64_t)p.c[2] << 32 | (uint64_t)p.c[3] << 48;
}
Px unpack(uint64_t v, int format) {
    Px p;
    const int bits = format == ZS_PNG_FMT_RGBA8 ? 8 : 16;
    for (int k = 0; k < 4; k++) p.c[k] = (uint32_t)(v >> (bits * k)) & ((1u << bits) - 1);
    return p;
}

long g_blends = 0, g_mixed = 0, g_anims = 0, g_wide_stores = 0;

bool check_blend(const Px &fg, const Px &bg, int format) {
    const uint64_t M = format == ZS_PNG_FMT_RGBA8 ? 255 : 65535;
    const Px want = over(fg, bg, M);
    const uint64_t got = format == ZS_PNG_FMT_RGBA8 ? png_blend_over<ZS_PNG_FMT_RGBA8>(pack(fg, format), pack(bg, format))
                                                    : png_blend_over<ZS_PNG_FMT_RGBA16>(pack(fg, format), pack(bg, format));
    g_blends++;
    if (fg.c[3] != 0 && fg.c[3] != M && bg.c[3] != 0) g_mixed++;
    if (!same(unpack(got, format), want)) {
        const Px g = unpack(got, format);
        printf("FAIL blend format %d: fg %u %u %u %u over bg %u %u %u %u: got %u %u %u %u, want %u %u %u %u\n", format, fg.c[0], fg.c[1], fg.c[2], fg.c[3],
               bg.c[0], bg.c[1], bg.c[2], bg.c[3], g.c[0], g.c[1], g.c[2], g.c[3], want.c[0], want.c[1], want.c[2], want.c[3]);
        return false;
    }
    // SOURCE is the frame's pixel whatever the canvas holds
    const uint64_t src = format == ZS_PNG_FMT_RGBA8 ? png_compose_blend<ZS_PNG_FMT_RGBA8>(0, pack(fg, format), pack(bg, format))
                                                    : png_compose_blend<ZS_PNG_FMT_RGBA16>(0, pack(fg, format), pack(bg, format));
    const uint64_t ovr = format == ZS_PNG_FMT_RGBA8 ? png_compose_blend<ZS_PNG_FMT_RGBA8>(1, pack(fg, format), pack(bg, format))
                                                    : png_compose_blend<ZS_PNG_FMT_RGBA16>(1, pack(fg, format), pack(bg, format));
    if (src != pack(fg, format) || ovr != got) return printf("FAIL png_compose_blend format %d\n", format), false;
    return true;
}

bool test_blend() {
    // RGBA8: every (fa, ba) pair with several colour pairs
    const uint32_t colors8[][2][3] = {{{0, 0, 0}, {255, 255, 255}}, {{255, 255, 255}, {0, 0, 0}}, {{255, 255, 255}, {255, 255, 255}}, {{1, 128, 254}, {254, 127, 1}},
                                      {{200, 100, 50}, {13, 77, 201}}, {{0, 1, 2}, {0, 1, 2}}};
    for (const auto &cp : colors8)
        for (uint32_t fa = 0; fa < 256; fa++)
            for (uint32_t ba = 0; ba < 256; ba++)
                if (!check_blend(Px{{cp[0][0], cp[0][1], cp[0][2], fa}}, Px{{cp[1][0], cp[1][1], cp[1][2], ba}}, ZS_PNG_FMT_RGBA8)) return false;
    // RGBA16: the edge values in every place, then random ones
    const uint32_t edge[7] = {0, 1, 257, 32767, 32768, 65534, 65535};
    for (uint32_t fa : edge)
        for (uint32_t ba : edge)
            for (uint32_t f : edge)
                for (uint32_t b : edge)
                    if (!check_blend(Px{{f, b, 65535 - f, fa}}, Px{{b, f, b, ba}}, ZS_PNG_FMT_RGBA16)) return false;
    std::mt19937_64 rng(20240611);
    for (int i = 0; i < 400000; i++) {
        Px fg, bg;
        for (int k = 0; k < 4; k++) fg.c[k] = (uint32_t)rng() & 65535, bg.c[k] = (uint32_t)rng() & 65535;
        if (i % 7 == 0) fg.c[3] = edge[rng() % 7];
        if (i % 11 == 0) bg.c[3] = edge[rng() % 7];
        if (!check_blend(fg, bg, ZS_PNG_FMT_RGBA16)) return false;
    }
    return true;
}

bool test_dispose() {
    for (int k = 0; k < 3; k++)
        for (int d = 0; d < 3; d++) {
            const uint64_t shown = 0x1122334455667788ull, before = 0x0102030405060708ull;
            // NONE keeps, BACKGROUND clears, PREVIOUS restores -- and clears on frame 0
            const uint64_t want = d == 0 ? shown : d == 1 ? 0 : k == 0 ? 0 : before;
            if (png_compose_dispose(d, k, shown, before) != want) return printf("FAIL dispose %d on frame %d\n", d, k), false;
        }
    return true;
}

// ---- whole animations ----
struct Frame {
    int x, y, w, h, dispose, blend;
    std::vector<uint8_t> px;  // h rows of w pixels, exactly
};
struct Anim {
    int w, h;
    std::vector<Frame> frames;
};

// frame by frame on a full canvas: canvases[k] is what is shown while frame k is up
std::vector<std::vector<Px>> restate(const Anim &a, int format) {
    const int P = png_expand_bytes(format);
    const uint64_t M = format == ZS_PNG_FMT_RGBA8 ? 255 : 65535;
    std::vector<Px> canvas((size_t)a.w * a.h, Px{{0, 0, 0, 0}});
    std::vector<std::vector<Px>> shown;
    for (size_t k = 0; k < a.frames.size(); k++) {
        const Frame &f = a.frames[k];
        const std::vector<Px> previous = canvas;
        for (int y = 0; y < f.h; y++)
            for (int x = 0; x < f.w; x++) {
                uint64_t raw = 0;
                memcpy(&raw, f.px.data() + ((size_t)y * f.w + x) * P, P);
                Px &dst = canvas[(size_t)(f.y + y) * a.w + f.x + x];
                const Px src = unpack(raw, format);
                dst = f.blend == 0 ? src : over(src, dst, M);
            }
        shown.push_back(canvas);
        for (int y = 0; y < f.h; y++)
            for (int x = 0; x < f.w; x++) {
                Px &dst = canvas[(size_t)(f.y + y) * a.w + f.x + x];
                if (f.dispose == 1 || (f.dispose == 2 && k == 0)) dst = Px{{0, 0, 0, 0}};
                else if (f.dispose == 2) dst = previous[(size_t)(f.y + y) * a.w + f.x + x];
            }
    }
    return shown;
}

template <int F>
void run_model(const PngComposeAnim &d, const std::vector<PngComposeFrame> &fr) {
    constexpr int N = kPngComposeGroup / png_expand_bytes(F);
    const int64_t ng = ((int64_t)d.width + N - 1) / N;
    // (rows and the lanes of a wave in any order: no group depends on another)
    for (int64_t y = d.height - 1; y >= 0; y--)
        for (int64_t g = ng - 1; g >= 0; g--) png_compose_group<F>(d, fr.data(), y, g * N);
}

bool run_anim(const Anim &a, int format, int residue) {
    const int P = png_expand_bytes(format);
    const size_t canvas = (size_t)a.w * a.h * P, total = canvas * a.frames.size();
    constexpr int kGuard = 64;
    std::vector<uint8_t> buf(total + 2 * kGuard + 32, 0xA5);
    uint8_t *base = buf.data() + kGuard;
    base += (16 - (uintptr_t)base % 16) % 16 + residue;  // (residue is a multiple of the pixel size)
    // the animation's frames are the second part of a longer list, as in a batch
    std::vector<PngComposeFrame> fr(3, PngComposeFrame{nullptr, 0, 0, 1, 1, 0, 0});
    for (const Frame &f : a.frames) fr.push_back(PngComposeFrame{f.px.data(), f.x, f.y, f.w, f.h, f.dispose, f.blend});
    const PngComposeAnim d{base, a.w, a.h, 3, (int32_t)a.frames.size()};
    if (format == ZS_PNG_FMT_RGBA8) run_model<ZS_PNG_FMT_RGBA8>(d, fr);
    else run_model<ZS_PNG_FMT_RGBA16>(d, fr);
    for (uint8_t *p = buf.data(); p < buf.data() + buf.size(); p++)
        if ((p < base || p >= base + total) && *p != 0xA5) return printf("FAIL guard: %dx%d format %d residue %d\n", a.w, a.h, format, residue), false;
    const auto want = restate(a, format);
    for (size_t k = 0; k < a.frames.size(); k++)
        for (int y = 0; y < a.h; y++)
            for (int x = 0; x < a.w; x++) {
                uint64_t raw = 0;
                memcpy(&raw, base + k * canvas + ((size_t)y * a.w + x) * P, P);
                if (!same(unpack(raw, format), want[k][(size_t)y * a.w + x])) {
                    const Px g = unpack(raw, format), &w = want[k][(size_t)y * a.w + x];
                    printf("FAIL canvas %zu of %zu, %dx%d format %d residue %d, pixel (%d, %d): got %u %u %u %u, want %u %u %u %u\n", k, a.frames.size(), a.w, a.h,
                           format, residue, x, y, g.c[0], g.c[1], g.c[2], g.c[3], w.c[0], w.c[1], w.c[2], w.c[3]);
                    return false;
                }
            }
    g_anims++;
    if (canvas % 16 == 0 && residue == 0 && a.w * P >= 16) g_wide_stores++;
    return true;
}

Anim random_anim(std::mt19937_64 &rng, int w, int h, int n_frames, int format) {
    const int P = png_expand_bytes(format);
    const uint32_t top = format == ZS_PNG_FMT_RGBA8 ? 255 : 65535;
    Anim a{w, h, {}};
    for (int k = 0; k < n_frames; k++) {
        Frame f;
        const int kind = (int)(rng() % 4);
        if (kind == 0) f.x = 0, f.y = 0, f.w = w, f.h = h;  // the whole canvas
        else {
            f.w = 1 + (int)(rng() % w), f.h = 1 + (int)(rng() % h);
            f.x = kind == 1 ? w - f.w : (int)(rng() % (w - f.w + 1));  // (touching the right and bottom edges)
            f.y = kind == 1 ? h - f.h : (int)(rng() % (h - f.h + 1));
        }
        f.dispose = (int)(rng() % 3), f.blend = (int)(rng() % 2);
        f.px.resize((size_t)f.w * f.h * P);
        for (int i = 0; i < f.w * f.h; i++) {
            Px p;
            for (int c = 0; c < 4; c++) p.c[c] = (uint32_t)rng() & top;
            const int r = (int)(rng() % 4);
            if (r == 0) p.c[3] = 0;
            else if (r == 1) p.c[3] = top;
            const uint64_t v = pack(p, format);
            memcpy(f.px.data() + (size_t)i * P, &v, P);
        }
        a.frames.push_back(f);
    }
    return a;
}

bool test_anims() {
    std::mt19937_64 rng(77);
    const int sizes[][2] = {{1, 1}, {2, 1}, {3, 2}, {4, 4}, {5, 3}, {7, 2}, {8, 3}, {17, 5}, {67, 4}, {261, 2}};
    for (int format = 0; format < 2; format++)
        for (const auto &s : sizes)
            for (int n_frames : {1, 2, 3, 9})
                for (int residue = 0; residue < 16; residue += png_expand_bytes(format))
                    if (!run_anim(random_anim(rng, s[0], s[1], n_frames, format), format, residue)) return false;
    // three PREVIOUS frames in a row behind a frame that stays, and PREVIOUS on frame 0
    for (int format = 0; format < 2; format++) {
        Anim a = random_anim(rng, 9, 4, 5, format);
        a.frames[0].dispose = 0;
        for (int k = 1; k < 4; k++) a.frames[(size_t)k].dispose = 2;
        if (!run_anim(a, format, 0)) return false;
        a.frames[0].dispose = 2;
        if (!run_anim(a, format, 8)) return false;
    }
    return true;
}

}  // namespace

int main() {
    if (!test_blend() || !test_dispose() || !test_anims()) return 1;
    if (g_mixed < 100000 || g_wide_stores == 0) return printf("FAIL coverage: %ld mixed blends, %ld animations with 16-byte stores\n", g_mixed, g_wide_stores), 1;
    printf("PASS %ld blends (%ld with both alphas partial), %ld animations\n", g_blends, g_mixed, g_anims);
    return 0;
}
