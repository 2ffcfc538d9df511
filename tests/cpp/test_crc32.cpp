// The CRC-32 code that the device kernels and the host share (zlibstream_amd/csrc/zs_crc32.h), run on the host:
//   * "123456789" gives 0xCBF43926;
//   * the byte step, the table form and the slice tables equal a bit-at-a-time loop on random buffers of every length 0..300;
//   * combine(crc(a), crc(b), |b|) == crc(a ++ b) for random splits, empty halves included, and for |b| up to 2^31 (against
//     zero bytes fed for real up to 2^24, and by associativity above that);
//   * the tile algebra of KC (zs_crc32.hip), both forms, restated with the same tables: 64 lanes over aligned 16-byte words
//     with a masked head, the lane fold by x^(128 q), the tail bytes, init and the bytes behind the tile -- every head
//     0..15 and a spread of lengths up to two tiles;
//   * the chunk walk on a few hand-made files.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_crc32.h"

using namespace zs;

static int fails = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (fails++ < 20) {               \
                printf("FAIL %s: ", #cond);   \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

static uint32_t crc_bitwise(uint32_t seed, const uint8_t *p, size_t n) {
    uint32_t c = ~seed;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

static std::vector<uint32_t> T;  // crc32_fill_tables
static uint32_t x2n[32];

static uint32_t raw16(const uint8_t *w) {
    uint32_t r = 0;
    for (int j = 0; j < 16; j++) r ^= T[kCrcTabSlice + (15 - j) * 256 + w[j]];
    return r;
}
static uint32_t shift_stride(uint32_t c) {
    uint32_t r = 0;
    for (int j = 0; j < 4; j++) r ^= T[kCrcTabShift + j * 256 + ((c >> (8 * j)) & 255)];
    return r;
}

// One tile as a wave of KC takes it: `base` 16-aligned, the tile is bytes [h, h + len) of it; returns what the wave XORs
// into the span's word.
static uint32_t tile_model(const uint8_t *base, int h, int len, bool strided, bool first, uint32_t init, uint32_t after) {
    const int end = h + len, NF = end >> 4, r = end & 15;
    uint32_t v = 0;
    for (int lane = 0; lane < 64; lane++) {
        uint32_t acc = 0;
        int e = NF;
        uint8_t w[16];
        auto word = [&](int m) {
            memcpy(w, base + 16 * m, 16);
            if (m == 0) memset(w, 0, (size_t)h);
        };
        if (strided) {
            for (int m = lane; m < NF; m += 64) word(m), acc = shift_stride(acc) ^ raw16(w), e = m + 1;
        } else {
            for (int m = lane * 8; m < lane * 8 + 8 && m < NF; m++) {
                word(m);
                for (int j = 0; j < 4; j++) w[j] ^= (uint8_t)(acc >> (8 * j));
                acc = raw16(w), e = m + 1;
            }
        }
        v ^= crc32_mul(acc, T[kCrcTabPow128 + (NF - e)]);
    }
    for (int i = NF ? 0 : h; i < r; i++) v = T[(v ^ base[16 * NF + i]) & 255] ^ (v >> 8);
    if (first && init) v ^= crc32_mul(crc32_mul(init, T[kCrcTabPow128 + (len >> 4)]), T[kCrcTabPow8 + (len & 15)]);
    if (after) {
        uint32_t f = kCrc32One;
        for (int k = 0; k < 32; k++)
            if ((after >> k) & 1) f = crc32_mul(f, T[kCrcTabX2n + ((k + 3) & 31)]);
        v = crc32_mul(v, f);
    }
    return v;
}

static uint32_t span_model(const uint8_t *p, int64_t len, uint32_t seed, bool strided) {
    // p sits at any offset of a buffer whose bytes around the span may be read
    uint32_t res = 0;
    for (int64_t t0 = 0; t0 < len; t0 += kCrcTile) {
        const int tl = (int)(len - t0 < kCrcTile ? len - t0 : kCrcTile);
        const uintptr_t a = (uintptr_t)(p + t0);
        const int h = (int)(a & 15);
        res ^= tile_model((const uint8_t *)(a - h), h, tl, strided, t0 == 0, ~seed, (uint32_t)(len - t0 - tl));
    }
    return ~(len > 0 ? res : ~seed);
}

static void put_chunk(std::vector<uint8_t> &f, const char *type, const std::vector<uint8_t> &data, bool good_crc = true) {
    uint8_t b[4];
    png_put_be32(b, (uint32_t)data.size());
    f.insert(f.end(), b, b + 4);
    const size_t at = f.size();
    f.insert(f.end(), type, type + 4);
    f.insert(f.end(), data.begin(), data.end());
    png_put_be32(b, crc_bitwise(0, f.data() + at, 4 + data.size()) ^ (good_crc ? 0 : 1));
    f.insert(f.end(), b, b + 4);
}

int main() {
    std::mt19937 rng(12345);
    T.resize(kCrcTabWords);
    crc32_fill_tables(T.data());
    crc32_x2n_table(x2n);
    const uint32_t *t0 = T.data();

    CHECK(crc32_bytes(t0, 0, (const uint8_t *)"123456789", 9) == 0xCBF43926u, "table form");
    CHECK(crc32_bytes_slow(0, (const uint8_t *)"123456789", 9) == 0xCBF43926u, "table-free form");
    for (int t = 0; t < 16; t++)
        for (uint32_t i = 0; i < 256; i += 17) CHECK(T[kCrcTabSlice + t * 256 + i] == crc32_table_entry(t, i), "slice %d entry %u", t, i);

    std::vector<uint8_t> buf((1 << 20) + 64);
    for (auto &b : buf) b = (uint8_t)rng();
    for (int len = 0; len <= 300; len++) {
        const uint8_t *p = buf.data() + (rng() % 1000);
        const uint32_t seed = len % 3 == 0 ? 0 : (uint32_t)rng();
        const uint32_t want = crc_bitwise(seed, p, (size_t)len);
        CHECK(crc32_bytes(t0, seed, p, (uint64_t)len) == want, "len %d", len);
        CHECK(crc32_bytes_slow(seed, p, (uint64_t)len) == want, "len %d (slow)", len);
        // continuing: the result fed back as the seed
        const int cut = len ? (int)(rng() % (unsigned)(len + 1)) : 0;
        CHECK(crc32_bytes(t0, crc32_bytes(t0, seed, p, (uint64_t)cut), p + cut, (uint64_t)(len - cut)) == want, "len %d cut %d", len, cut);
    }

    // combine
    for (int it = 0; it < 400; it++) {
        const size_t n = it < 8 ? (size_t)it : rng() % 5000, cut = it % 7 == 0 ? 0 : it % 7 == 1 ? n : rng() % (n + 1);
        const uint8_t *p = buf.data() + (rng() % 1000);
        const uint32_t a = crc_bitwise(0, p, cut), b = crc_bitwise(0, p + cut, n - cut);
        CHECK(crc32_combine(x2n, a, b, n - cut) == crc_bitwise(0, p, n), "combine n %zu cut %zu", n, cut);
    }
    {
        // long second halves: zero bytes fed for real up to 2^24 ...
        std::vector<uint8_t> zeros(1 << 24, 0);
        const uint32_t a = crc_bitwise(0, buf.data(), 1000);
        uint32_t run = a;
        size_t fed = 0;
        for (int k = 10; k <= 24; k++) {
            const size_t n = (size_t)1 << k;
            run = crc32_bytes(t0, run, zeros.data(), n - fed);  // a ++ zeros(n)
            fed = n;
            CHECK(crc32_combine(x2n, a, crc32_bytes(t0, 0, zeros.data(), n), n) == run, "zeros 2^%d", k);
        }
        // ... and above that by associativity: (a ++ b1) ++ b2 == a ++ (b1 ++ b2), |b1| + |b2| up to 2^31
        const uint32_t b1 = (uint32_t)rng(), b2 = (uint32_t)rng();
        for (int it = 0; it < 64; it++) {
            const uint64_t total = it == 0 ? (uint64_t)1 << 31 : it == 1 ? ((uint64_t)1 << 31) - 1 : ((uint64_t)rng() << 1 | 1) & 0x7FFFFFFFu;
            const uint64_t l2 = it % 5 == 0 ? 0 : rng() % (total + 1), l1 = total - l2;
            const uint32_t left = crc32_combine(x2n, crc32_combine(x2n, a, b1, l1), b2, l2);
            const uint32_t right = crc32_combine(x2n, a, crc32_combine(x2n, b1, b2, l2), total);
            CHECK(left == right, "associativity total %llu l2 %llu", (unsigned long long)total, (unsigned long long)l2);
        }
        // x^(8 * 2^31) against 31 squarings of x^8 done here
        uint32_t p = crc32_xpow(x2n, 1, 3);
        for (int k = 0; k < 31; k++) p = crc32_mul(p, p);
        CHECK(crc32_xpow(x2n, (uint64_t)1 << 31, 3) == p, "x^(8 * 2^31)");
    }

    // the tile algebra, both forms
    {
        std::vector<int> lens;
        for (int l = 0; l <= 130; l++) lens.push_back(l);
        for (int l : {1023, 1024, 1025, 2047, 2049, kCrcTile - 17, kCrcTile - 1, kCrcTile, kCrcTile + 1, 2 * kCrcTile + 1, kCrcWaves * kCrcTile - 1, kCrcWaves * kCrcTile + 1, 100000})
            lens.push_back(l);
        uint8_t *al = buf.data() + ((16 - ((uintptr_t)buf.data() & 15)) & 15) + 16;
        std::vector<uint8_t> ff(buf.size(), 0xFF);
        uint8_t *alf = ff.data() + ((16 - ((uintptr_t)ff.data() & 15)) & 15) + 16;
        for (int h = 0; h < 16; h++)
            for (int len : lens)
                for (int form = 0; form < 2; form++) {
                    const uint32_t seed = (h + len) % 3 == 0 ? 0u : (h + len) % 3 == 1 ? 0xFFFFFFFFu : 0x35AF061Eu;
                    CHECK(span_model(al + h, len, seed, form == 0) == crc_bitwise(seed, al + h, (size_t)len), "tile model h %d len %d form %d", h, len, form);
                    if (len < 3000 || h == 5) CHECK(span_model(alf + h, len, seed, form == 0) == crc_bitwise(seed, alf + h, (size_t)len), "tile model 0xFF h %d len %d form %d", h, len, form);
                }
    }

    // bound and chunk walk
    CHECK(png_file_bound(0, 0, 0) == 8 + 25 + 12 + 12, "bound of nothing");
    CHECK(png_file_bound(8193, 8192, 5) == 8 + 25 + 5 + 8193 + 24 + 12, "bound, two chunks");
    CHECK(png_file_bound(-1, 0, 0) == -1 && png_file_bound(1, -1, 0) == -1 && png_file_bound(1, (int64_t)1 << 31, 0) == -1 && png_file_bound(1, 0, -1) == -1, "bad bounds");
    {
        static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
        std::vector<uint8_t> ihdr = {0, 0, 0, 5, 0, 0, 0, 3, 8, 2, 0, 0, 0};
        std::vector<uint8_t> f(sig, sig + 8);
        put_chunk(f, "IHDR", ihdr);
        put_chunk(f, "gAMA", {0, 1, 2, 3}, false);  // an ancillary chunk's CRC is not read
        put_chunk(f, "IDAT", {1, 2, 3});
        put_chunk(f, "IDAT", {});
        put_chunk(f, "IDAT", {4});
        put_chunk(f, "tEXt", {9});
        const size_t before_end = f.size();
        put_chunk(f, "IEND", {});
        PngFileInfo info;
        char msg[160];
        int seen = 0;
        CHECK(png_walk_file(f.data(), (int64_t)f.size(), &info, msg, sizeof msg, true, [&](const PngChunkRef &) { seen++; }), "%s", msg);
        CHECK(info.width == 5 && info.height == 3 && info.bit_depth == 8 && info.color_type == 2 && info.interlace == 0 && info.bits_per_pixel == 24, "IHDR fields");
        CHECK(info.idat_bytes == 4 && info.n_idat == 3 && info.pixel_bytes == 45 && seen == 5, "chain: %lld %lld %lld %d", (long long)info.idat_bytes, (long long)info.n_idat, (long long)info.pixel_bytes, seen);
        CHECK(png_chunks_well_formed(f.data() + 8, (int64_t)f.size() - 8) && !png_chunks_well_formed(f.data() + 8, (int64_t)f.size() - 9), "well-formed");
        auto bad = [&](std::vector<uint8_t> g, const char *what) {
            CHECK(!png_walk_file(g.data(), (int64_t)g.size(), &info, msg, sizeof msg, true, [](const PngChunkRef &) {}), "%s accepted", what);
            CHECK(strstr(msg, what) != nullptr, "'%s' lacks '%s'", msg, what);
        };
        std::vector<uint8_t> g = f;
        g[0] = 0x88;
        bad(g, "signature");
        g = f, g.resize(f.size() - 3);
        bad(g, "truncated");
        g = f, g.resize(before_end);
        bad(g, "IEND is missing");
        g = f, g[8 + 8 + 9] = 5;  // color type 5
        bad(g, "CRC error in IHDR");
        g = f, g[8 + 25 + 16 + 8 + 1] ^= 0x40;  // inside the first IDAT's data
        bad(g, "CRC error in IDAT");
        g.assign(sig, sig + 8);
        put_chunk(g, "gAMA", {0, 1, 2, 3});
        put_chunk(g, "IHDR", ihdr);
        bad(g, "IHDR is not the first");
        g.assign(sig, sig + 8);
        put_chunk(g, "IHDR", ihdr), put_chunk(g, "IEND", {});
        bad(g, "no IDAT");
        g.assign(sig, sig + 8);
        put_chunk(g, "IHDR", ihdr), put_chunk(g, "IDAT", {1}), put_chunk(g, "tEXt", {}), put_chunk(g, "IDAT", {2}), put_chunk(g, "IEND", {});
        bad(g, "not consecutive");
        for (auto ct_bd : {std::pair<int, int>{2, 4}, {3, 16}, {4, 2}, {6, 1}, {1, 8}, {0, 3}}) {
            ihdr[9] = (uint8_t)ct_bd.first, ihdr[8] = (uint8_t)ct_bd.second;
            g.assign(sig, sig + 8);
            put_chunk(g, "IHDR", ihdr), put_chunk(g, "IDAT", {1}), put_chunk(g, "IEND", {});
            bad(g, "color type");
        }
        ihdr[9] = 2, ihdr[8] = 8, ihdr[12] = 2;
        g.assign(sig, sig + 8);
        put_chunk(g, "IHDR", ihdr), put_chunk(g, "IDAT", {1}), put_chunk(g, "IEND", {});
        bad(g, "interlace 2");
        ihdr[12] = 0, ihdr[3] = 0;  // width 0
        g.assign(sig, sig + 8);
        put_chunk(g, "IHDR", ihdr), put_chunk(g, "IDAT", {1}), put_chunk(g, "IEND", {});
        bad(g, "width or height");
    }
    if (fails) {
        printf("FAILED: %d checks\n", fails);
        return 1;
    }
    printf("PASS\n");
    return 0;
}
