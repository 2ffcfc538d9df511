// test_exr_walk.cpp -- the OpenEXR rules of zlibstream_amd/csrc/zs_exr.h on the host, built with -fsanitize=address,undefined
// by tests/test_exr_host.py:
//   - exr_walk on every file given on the command line (tests/exr_cases.py builds them: scanlines and tiles, ZIP, ZIPS and
//     none, a negative origin, decreasing order) and on every prefix of each, every one in a heap block of exactly its length,
//     so that a read past the end is the sanitizer's to report; a prefix never gives more chunks than the whole file, and a
//     chunk it calls whole lies inside it;
//   - the writer's head read back by the walk;
//   - the predictor kernels' per-lane step (exr_group_sum, exr_lane_scan, exr_lane_finish, exr_interleave, exr_split,
//     exr_lane_diff, exr_find_run) over a model of the wave -- 64 lanes of 16-byte groups of each half, tiles of kExrSeg bytes
//     of each half whose carries come from segment sums, as zs_exr.hip runs them -- against a scalar loop.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_exr.h"

using namespace zs;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (++failures < 20) {            \
                printf("FAIL %s: ", #cond);   \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

// the walk of `len` bytes of the file, in a block of exactly that size
static int walk_exact(const std::vector<uint8_t> &file, int64_t len, ExrInfo *info, std::vector<ExrChannel> *ch, std::vector<ExrChunk> *chunks) {
    uint8_t *block = (uint8_t *)malloc((size_t)len ? (size_t)len : 1);
    memcpy(block, file.data(), (size_t)len);
    int rc = exr_walk(block, len, info, nullptr, 0, nullptr, 0);
    if (rc == kExrOk) {
        ch->assign((size_t)info->n_channels, ExrChannel{});
        chunks->assign((size_t)info->n_chunks, ExrChunk{});
        rc = exr_walk(block, len, info, ch->data(), info->n_channels, chunks->data(), info->n_chunks);
    }
    free(block);
    return rc;
}

static void test_file(const char *path) {
    const std::vector<uint8_t> file = slurp(path);
    CHECK(!file.empty(), "%s", path);
    ExrInfo whole;
    std::vector<ExrChannel> wch;
    std::vector<ExrChunk> wc;
    const int rc = walk_exact(file, (int64_t)file.size(), &whole, &wch, &wc);
    CHECK(rc == kExrOk, "%s: %d %s", path, rc, exr_err_message(rc));
    for (const ExrChunk &c : wc) CHECK(c.status == 0 && c.off + c.data_len <= (int64_t)file.size() && c.w >= 1 && c.h >= 1, "%s", path);
    int64_t ok_before = 0;
    for (int64_t len = 0; len <= (int64_t)file.size(); len++) {
        ExrInfo ei;
        std::vector<ExrChannel> ch;
        std::vector<ExrChunk> cs;
        const int r = walk_exact(file, len, &ei, &ch, &cs);
        if (len < 8) CHECK(r == kExrShortFile, "%s cut %lld: %d", path, (long long)len, r);
        if (r != kExrOk) {
            CHECK(ok_before == 0 && (r == kExrShortFile || r == kExrHeaderOut || r == kExrTableOut), "%s cut %lld: %d", path, (long long)len, r);
            continue;
        }
        CHECK(ei.n_chunks == whole.n_chunks && ei.out_len == whole.out_len && ei.n_channels == whole.n_channels, "%s cut %lld", path, (long long)len);
        int64_t ok = 0;
        for (const ExrChunk &c : cs) {
            if (c.status == 0) {
                CHECK(c.off >= 0 && c.data_len >= 0 && c.off + c.data_len <= len, "%s cut %lld", path, (long long)len);
                ok++;
            } else {
                CHECK(c.status == -5 && c.reason == kExrTruncated, "%s cut %lld: %d", path, (long long)len, c.status);
            }
            CHECK(c.x + c.w <= ei.width && c.y + c.h <= ei.height, "%s cut %lld", path, (long long)len);
        }
        CHECK(ok >= ok_before, "%s cut %lld: fewer whole chunks than a shorter prefix has", path, (long long)len);
        ok_before = ok;
    }
    CHECK(ok_before == whole.n_chunks, "%s", path);
}

static void test_writer() {
    const char *names[3] = {"A", "Zdepth", "r.long-ish_name"};
    const int types[3] = {1, 2, 0};
    const uint8_t extra[] = {'o', 'w', 'n', 'e', 'r', 0, 's', 't', 'r', 'i', 'n', 'g', 0, 2, 0, 0, 0, 'm', 'e'};
    for (int compression : {0, 2, 3}) {
        ExrLayout l{};
        l.width = 7, l.height = 37, l.x_min = -3, l.y_min = -20, l.n_channels = 3, l.compression = compression, l.names = names, l.types = types;
        l.extra = extra, l.extra_len = (int64_t)sizeof extra;
        l.bpp = 10, l.n_chunks = exr_ceil_div(l.height, exr_lines(compression));
        std::vector<int64_t> body((size_t)l.n_chunks), off((size_t)l.n_chunks);
        for (int64_t k = 0; k < l.n_chunks; k++) {
            const int64_t rows = std::min<int64_t>(exr_lines(compression), l.height - k * exr_lines(compression));
            body[(size_t)k] = rows * l.width * l.bpp;  // (stored raw)
        }
        const int64_t head = exr_head_bytes(l);
        uint8_t *p = (uint8_t *)malloc((size_t)head);
        const int64_t total = exr_put_head(p, l, body.data(), off.data());
        uint8_t *file = (uint8_t *)calloc(1, (size_t)total);
        memcpy(file, p, (size_t)head);
        free(p);
        CHECK(off[0] == head, "compression %d", compression);
        for (int64_t k = 0; k < l.n_chunks; k++) {
            exr_put32(file + off[(size_t)k], (uint32_t)(l.y_min + (int32_t)(k * exr_lines(compression))));
            exr_put32(file + off[(size_t)k] + 4, (uint32_t)body[(size_t)k]);
        }
        ExrInfo ei;
        std::vector<ExrChannel> ch(3);
        std::vector<ExrChunk> cs((size_t)l.n_chunks);
        const int rc = exr_walk(file, total, &ei, ch.data(), 3, cs.data(), l.n_chunks);
        CHECK(rc == kExrOk, "compression %d: %d %s", compression, rc, exr_err_message(rc));
        CHECK(ei.width == 7 && ei.height == 37 && ei.n_channels == 3 && ei.compression == compression && ei.line_order == 0 && !ei.tiled && ei.n_chunks == l.n_chunks, "info");
        CHECK(ei.data_window[0] == -3 && ei.data_window[1] == -20 && ei.data_window[2] == 3 && ei.data_window[3] == 16 && ei.has_display_window && ei.display_window[3] == 16, "windows");
        CHECK(!strcmp(ch[0].name, "A") && !strcmp(ch[1].name, "Zdepth") && !strcmp(ch[2].name, names[2]) && ch[1].type == 2 && ch[2].sample_bytes == 4, "channels");
        CHECK(ch[0].plane_off == 0 && ch[1].plane_off == ((7 * 37 * 2 + 15) & ~15) && ei.out_len == ch[2].plane_off + 7 * 37 * 4, "planes");
        for (int64_t k = 0; k < l.n_chunks; k++)
            CHECK(cs[(size_t)k].status == 0 && cs[(size_t)k].off == off[(size_t)k] + 8 && cs[(size_t)k].data_len == body[(size_t)k] && cs[(size_t)k].raw_len == body[(size_t)k], "chunk %lld", (long long)k);
        CHECK(cs.back().off + cs.back().data_len == total, "the file's length");
        free(file);
    }
}

// ---- the wave model
static void load16(const uint8_t *p, int64_t pos, int64_t end, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    for (int64_t b = pos; b < end && b < pos + 16; b++) w[(b - pos) >> 2] |= (uint32_t)p[b] << (8 * ((b - pos) & 3));
}
static void store16(uint8_t *p, int64_t pos, int64_t end, const uint32_t w[4]) {
    for (int64_t b = pos; b < end && b < pos + 16; b++) p[b] = (uint8_t)(w[(b - pos) >> 2] >> (8 * ((b - pos) & 3)));
}

// the undo as the kernels run it: segment sums, then per tile the carries and the passes
static std::vector<uint8_t> model_undo(const std::vector<uint8_t> &t) {
    const int64_t U = (int64_t)t.size(), h = (U + 1) >> 1, n_tiles = exr_tiles(U);
    std::vector<uint8_t> seg((size_t)(2 * n_tiles), 0), raw((size_t)U, 0xEE);
    for (int64_t q = 0; q < n_tiles; q++) {
        uint32_t tot1 = 0, tot2 = 0;
        for (int lane = 0; lane < 64; lane++) {
            uint32_t s1 = 0, s2 = 0;
            for (int64_t pos = q * kExrSeg + 16 * lane; pos < (q + 1) * (int64_t)kExrSeg; pos += kExrPass) {
                uint32_t w[4];
                if (pos < h) load16(t.data(), pos, h, w), s1 = exr_add8(s1, exr_group_sum(w));
                if (pos < U - h) load16(t.data() + h, pos, U - h, w), s2 = exr_add8(s2, exr_group_sum(w));
            }
            tot1 += exr_fold8(s1) & 0xFF, tot2 += exr_fold8(s2) & 0xFF;
        }
        seg[(size_t)q] = (uint8_t)tot1, seg[(size_t)(n_tiles + q)] = (uint8_t)tot2;
    }
    for (int64_t q = 0; q < n_tiles; q++) {
        uint32_t c1 = 0, c2 = 0;
        for (int64_t k = 0; k < n_tiles + q; k++) c2 += seg[(size_t)k], c1 += k < q ? seg[(size_t)k] : 0;
        for (int64_t base = q * kExrSeg; base < (q + 1) * (int64_t)kExrSeg && base < h; base += kExrPass) {
            uint32_t wa[64][4], wb[64][4], ta[64], tb[64];
            for (int lane = 0; lane < 64; lane++) {
                load16(t.data(), base + 16 * lane, h, wa[lane]), load16(t.data() + h, base + 16 * lane, U - h, wb[lane]);
                ta[lane] = exr_lane_scan(wa[lane]) & 0xFF, tb[lane] = exr_lane_scan(wb[lane]) & 0xFF;
            }
            uint32_t ua = 0, ub = 0;  // the wave scan: the totals of the lanes up to this one
            for (int lane = 0; lane < 64; lane++) {
                ua += ta[lane], ub += tb[lane];
                exr_lane_finish(wa[lane], c1 + ua - ta[lane], 0);
                exr_lane_finish(wb[lane], c2 + ub - tb[lane], (int)(h & 1));
                uint32_t out[8];
                exr_interleave(wa[lane], wb[lane], out);
                const int64_t pos = 2 * (base + 16 * lane);
                store16(raw.data(), pos, U, out), store16(raw.data(), pos + 16, U, out + 4);
            }
            c1 += ua, c2 += ub;
        }
    }
    return raw;
}

static std::vector<uint8_t> model_predict(const std::vector<uint8_t> &raw) {
    const int64_t U = (int64_t)raw.size(), h = (U + 1) >> 1;
    std::vector<uint8_t> t((size_t)U, 0xEE);
    for (int64_t base = 0; base < h; base += kExrPass) {
        uint32_t last = 0;
        for (int lane = 0; lane < 64; lane++) {
            const int64_t pos = base + 16 * lane, in = 2 * pos;
            uint32_t r[8], wa[4], wb[4];
            load16(raw.data(), in, U, r), load16(raw.data(), in + 16, U, r + 4);
            uint32_t before = last >> 16;
            if (lane == 0) {
                if (base == 0) before = 128 | (U > 1 ? (uint32_t)raw[(size_t)(2 * (h - 1))] : 0) << 8;
                else before = raw[(size_t)(in - 2)] | (uint32_t)raw[(size_t)(in - 1)] << 8;
            }
            last = r[7];
            exr_split(r, wa, wb);
            exr_lane_diff(wa, before & 0xFF), exr_lane_diff(wb, before >> 8);
            store16(t.data(), pos, h, wa), store16(t.data() + h, pos, U - h, wb);
        }
    }
    return t;
}

static void test_lane_step() {
    const int64_t lens[] = {1, 2, 3, 31, 32, 33, 1023, 1025, 3 * (int64_t)kExrTile + 1};
    uint32_t seed = 12345;
    for (int64_t U : lens) {
        for (int fill = 0; fill < 2; fill++) {
            std::vector<uint8_t> raw((size_t)U);
            for (auto &b : raw) seed = seed * 1664525u + 1013904223u, b = fill ? 0xFF : (uint8_t)(seed >> 24);
            // the scalar rule
            const int64_t h = (U + 1) / 2;
            std::vector<uint8_t> split((size_t)U), want((size_t)U);
            for (int64_t k = 0; k < U; k++) split[(size_t)(k % 2 ? h + k / 2 : k / 2)] = raw[(size_t)k];
            want[0] = split[0];
            for (int64_t i = 1; i < U; i++) want[(size_t)i] = (uint8_t)(split[(size_t)i] - split[(size_t)(i - 1)] + 128);
            const std::vector<uint8_t> t = model_predict(raw);
            CHECK(t == want, "forward, U = %lld fill %d", (long long)U, fill);
            CHECK(model_undo(want) == raw, "undo, U = %lld fill %d", (long long)U, fill);
            // stored bytes of all 0xFF: every sum wraps
            std::vector<uint8_t> ff((size_t)U, 0xFF), back((size_t)U);
            uint8_t s = 0;
            std::vector<uint8_t> sums((size_t)U);
            for (int64_t i = 0; i < U; i++) s = (uint8_t)(i ? s + 0xFF - 128 : 0xFF), sums[(size_t)i] = s;
            for (int64_t k = 0; k < U; k++) back[(size_t)k] = sums[(size_t)(k % 2 ? h + k / 2 : k / 2)];
            CHECK(model_undo(ff) == back, "undo of 0xFF, U = %lld", (long long)U);
        }
    }
    // the run search: the last run that begins at or in front of the byte
    ExrRun runs[5] = {{nullptr, 0, 4}, {nullptr, 4, 1}, {nullptr, 5, 10}, {nullptr, 15, 2}, {nullptr, 17, 3}};
    const int want[20] = {0, 0, 0, 0, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 4, 4, 4};
    for (int pos = 0; pos < 20; pos++) CHECK(exr_find_run(runs, 5, pos) == want[pos], "run of %d", pos);
    CHECK(exr_find_run(runs, 1, 3) == 0, "one run");
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; i++) test_file(argv[i]);
    test_writer();
    test_lane_step();
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("PASS\n");
    return 0;
}
