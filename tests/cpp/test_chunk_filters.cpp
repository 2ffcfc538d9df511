// test_chunk_filters.cpp -- the filter rules of zlibstream_amd/csrc/zs_chunk.h on the host, built with
// -fsanitize=address,undefined by tests/test_chunk_filter_host.py:
//   * Fletcher-32: the closed form (a tile's sums by the per-lane step of the kernel, lanes 0..63 one after the other, tiles
//     combined by the rule of the header and by the fold's sum) against the literal loop of H5_checksum_fletcher32 -- every
//     input of 0..5 bytes over {0x00, 0x01, 0xfe, 0xff}, all-zero and all-0xff inputs at the lengths where the loop folds, 200
//     random inputs, every start address modulo 16, lengths around one and two tiles, and the combine rule at every cut;
//   * the rules of a (grid, filters) pair from both sides;
//   * delta: the encode step and the three decode steps over a model of the wave against a scalar loop, elem_size 1, 2, 4, 8,
//     plain, shuffled and big-endian chunk sides, counts around a lane's unit, a pass and a tile, with leftover bytes;
//   * the byte reversal of the place and gather steps, shuffled and plain, rows of every lane unit, with padding.
// Every buffer but the aligned tile copies is a heap block of exactly its length.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_chunk.h"

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

static uint32_t rng_state = 4321;
static uint32_t rnd32() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}
static uint8_t rnd() { return (uint8_t)rnd32(); }

struct Block {  // a heap block of exactly n bytes
    std::unique_ptr<uint8_t[]> p;
    int64_t n;
    explicit Block(int64_t len) : p(new uint8_t[(size_t)(len ? len : 1)]), n(len) {}
    uint8_t *get() { return p.get(); }
};

// ------------------------------------------------------------------ Fletcher-32
static uint32_t fletcher_loop(const uint8_t *d, size_t len) {  // H5_checksum_fletcher32
    uint32_t s1 = 0, s2 = 0;
    size_t words = len / 2, p = 0;
    while (words) {
        size_t t = words > 360 ? 360 : words;
        words -= t;
        do {
            s1 += ((uint32_t)d[p] << 8) | d[p + 1];
            p += 2;
            s2 += s1;
        } while (--t);
        s1 = (s1 & 0xffff) + (s1 >> 16);
        s2 = (s2 & 0xffff) + (s2 >> 16);
    }
    if (len % 2) {
        s1 += (uint32_t)d[p] << 8;
        s2 += s1;
        s1 = (s1 & 0xffff) + (s1 >> 16);
        s2 = (s2 & 0xffff) + (s2 >> 16);
    }
    s1 = (s1 & 0xffff) + (s1 >> 16);
    s2 = (s2 & 0xffff) + (s2 >> 16);
    return (s2 << 16) | s1;
}

// a run of bytes as the tile kernel sees it: h bytes into a 16-byte word, the lanes one after the other
static FletSum tile_sum(const uint8_t *d, int len, int h) {
    const int words = (h + len + 15) >> 4;
    std::vector<uint8_t> buf((size_t)words * 16 + 16, 0xA5);  // (what lies around the tile in its words must not count)
    uint8_t *base = buf.data() + ((16 - ((uintptr_t)buf.data() & 15)) & 15);
    if (len) memcpy(base + h, d, (size_t)len);
    uint64_t a1 = 0, a2 = 0;
    bool nz = false;
    for (int lane = 0; lane < 64; lane++) {
        uint64_t A1 = 0, A2 = 0;
        fletcher_tile_lane(base, h, len, lane, &A1, &A2);
        nz = nz || A1 != 0;
        a1 += A1 % 65535u, a2 += A2 % 65535u;
    }
    return FletSum{(uint32_t)(a1 % 65535u), (uint32_t)(a2 % 65535u), nz ? 1u : 0u, 0};
}

// the whole span: tiles of `tile` bytes combined one after the other by the rule, and added up as the fold kernel does
static void check_span(const uint8_t *d, int64_t len, int h, int tile, const char *what) {
    const uint32_t want = fletcher_loop(d, (size_t)len);
    const int64_t words = (len + 1) / 2, tiles = (len + tile - 1) / tile;
    FletSum run{0, 0, 0, 0};
    uint64_t B1 = 0, B2 = 0;
    uint32_t any = 0;
    for (int64_t t = 0; t < tiles; t++) {
        const int n = (int)(len - t * tile < tile ? len - t * tile : tile);
        const FletSum s = tile_sum(d + t * tile, n, (h + (int)((t * tile) & 15)) & 15);
        run = fletcher_combine(run, s, (n + 1) / 2);
        const int64_t behind = t + 1 < tiles ? words - (t + 1) * (tile / 2) : 0;
        B1 += s.a1, B2 += s.a2 + (uint64_t)(behind % 65535) * s.a1, any |= s.nz;
    }
    const FletSum fold{(uint32_t)(B1 % 65535u), (uint32_t)(B2 % 65535u), any, 0};
    CHECK(fletcher_finish(run) == want, "%s: len %lld h %d tile %d: combined %08x, loop %08x", what, (long long)len, h, tile, fletcher_finish(run), want);
    CHECK(fletcher_finish(fold) == want, "%s: len %lld h %d tile %d: folded %08x, loop %08x", what, (long long)len, h, tile, fletcher_finish(fold), want);
}

static void test_fletcher() {
    const uint8_t alphabet[4] = {0x00, 0x01, 0xfe, 0xff};
    for (int len = 0; len <= 5; len++) {
        int total = 1;
        for (int i = 0; i < len; i++) total *= 4;
        for (int v = 0; v < total; v++) {
            Block b(len);
            for (int i = 0, x = v; i < len; i++, x /= 4) b.get()[i] = alphabet[x % 4];
            check_span(b.get(), len, v & 15, kFletTile, "alphabet");
            check_span(b.get(), len, 0, 2, "alphabet, tiles of a word");
        }
    }
    const int lens[] = {0, 1, 2, 3, 719, 720, 721, 722, 1439, 1440, 1441, 1442, 65534, 65535, 65536, 65537, 65538, kFletTile - 1, kFletTile, kFletTile + 1, 2 * kFletTile + 1};
    for (int len : lens)
        for (int fill = 0; fill < 2; fill++) {
            Block b(len);
            memset(b.get(), fill ? 0xff : 0x00, (size_t)len);
            check_span(b.get(), len, len & 15, kFletTile, fill ? "all 0xff" : "all zero");
            check_span(b.get(), len, 3, 720, fill ? "all 0xff, tiles of 720" : "all zero, tiles of 720");
        }
    for (int k = 0; k < 200; k++) {
        const int len = (int)(rnd32() % 4097);
        Block b(len);
        for (int i = 0; i < len; i++) b.get()[i] = rnd();
        check_span(b.get(), len, k & 15, kFletTile, "random");
        check_span(b.get(), len, (k >> 4) & 15, 2 * (1 + (int)(rnd32() % 300)), "random, small tiles");
    }
    for (int h = 0; h < 16; h++)
        for (int len : {kFletTile - 1, kFletTile, kFletTile + 1, 2 * kFletTile + 1, 40001}) {
            Block b(len);
            for (int i = 0; i < len; i++) b.get()[i] = rnd();
            check_span(b.get(), len, h, kFletTile, "random at every address");
        }
    // the combine rule at every even cut of three inputs, one of them with an odd length and one all 0xff
    for (int which = 0; which < 3; which++) {
        const int len = which == 0 ? 1441 : which == 1 ? 722 : 2000;
        Block b(len);
        for (int i = 0; i < len; i++) b.get()[i] = which == 1 ? 0xff : rnd();
        const uint32_t want = fletcher_loop(b.get(), (size_t)len);
        for (int cut = 0; cut <= len; cut += 2) {
            const FletSum a = tile_sum(b.get(), cut, 0), c = tile_sum(b.get() + cut, len - cut, cut & 15);
            const uint32_t got = fletcher_finish(fletcher_combine(a, c, (len - cut + 1) / 2));
            CHECK(got == want, "cut %d of %d: %08x, loop %08x", cut, len, got, want);
        }
    }
}

// ------------------------------------------------------------------ the rules of a pair
static void test_rules() {
    for (int es = 1; es <= 16; es++) {
        const bool pow2 = es == 1 || es == 2 || es == 4 || es == 8;
        CHECK(chunk_filters_check(es, ChunkFilters{0, 0, 0, 0}) && chunk_filters_check(es, ChunkFilters{0, 0, 1, 0}), "es %d without delta", es);
        CHECK(chunk_filters_check(es, ChunkFilters{1, 0, 0, 0}) == pow2 && chunk_filters_check(es, ChunkFilters{0, 1, 0, 0}) == pow2, "es %d", es);
    }
    for (int field = 0; field < 3; field++)
        for (int v : {-1, 2}) {
            int f[4] = {0, 0, 0, 0};
            f[field] = v;
            CHECK(!chunk_filters_check(4, ChunkFilters{f[0], f[1], f[2], f[3]}), "field %d = %d", field, v);
        }
    CHECK(!chunk_filters_check(4, ChunkFilters{0, 0, 0, 1}) && chunk_filters_check(4, ChunkFilters{1, 1, 1, 0}), "reserved");
}

// ------------------------------------------------------------------ delta
static uint64_t get_le(const uint8_t *p, int es) {
    uint64_t v = 0;
    for (int j = 0; j < es; j++) v |= (uint64_t)p[j] << (8 * j);
    return v;
}
// element k of a chunk side
static uint8_t *side_byte(uint8_t *p, int64_t E, int es, int flags, int64_t k, int j) {
    const int sj = (flags & kDeltaSwap) && es > 1 ? es - 1 - j : j;
    return (flags & kDeltaShuffled) && es > 1 ? p + sj * E + k : p + k * es + sj;
}

template <int ES>
static void delta_case(int64_t E, int left, int flags) {
    const int64_t n = E * ES + left;
    Block plain(n), side(n), enc(n), dec(n);
    for (int64_t i = 0; i < n; i++) plain.get()[i] = (i / ES) % 7 == 0 ? 0xff : rnd();  // (runs of 0xff.. followed by small values wrap)
    // the scalar model: differences into the chunk side
    for (int64_t k = 0; k < E; k++) {
        const uint64_t d = get_le(plain.get() + k * ES, ES) - (k ? get_le(plain.get() + (k - 1) * ES, ES) : 0);
        for (int j = 0; j < ES; j++) *side_byte(side.get(), E, ES, flags, k, j) = (uint8_t)(d >> (8 * j));
    }
    memcpy(side.get() + E * ES, plain.get() + E * ES, (size_t)left);
    const int64_t tiles = delta_tiles(E, left);
    // encode
    memset(enc.get(), 0x5A, (size_t)n);
    DeltaJob je{plain.get(), enc.get(), E, ES, flags, left, 0};
    for (int64_t t = 0; t < tiles; t++)
        for (int lane = 0; lane < 64; lane++) {
            for (int pass = 0; pass < kDeltaPasses; pass++) delta_encode_lane<ES>(je, t, pass, lane);
            delta_copy_left(je, t, lane);
        }
    CHECK(memcmp(enc.get(), side.get(), (size_t)n) == 0, "encode: E %lld es %d flags %d left %d", (long long)E, ES, flags, left);
    // decode: tile sums, their scan, the tiles again
    memset(dec.get(), 0x5A, (size_t)n);
    DeltaJob jd{side.get(), dec.get(), E, ES, flags, left, 0};
    std::vector<uint64_t> sums((size_t)tiles, 0);
    for (int64_t t = 0; t < tiles; t++)
        for (int lane = 0; lane < 64; lane++)
            for (int pass = 0; pass < kDeltaPasses; pass++) {
                uint64_t x[kDeltaUnit];
                int64_t e;
                int cnt;
                sums[(size_t)t] += delta_decode_load<ES>(jd, t, pass, lane, x, &e, &cnt);
            }
    uint64_t carry = 0;
    for (int64_t t = 0; t < tiles; t++) {
        const uint64_t v = sums[(size_t)t];
        sums[(size_t)t] = carry, carry += v;
    }
    for (int64_t t = 0; t < tiles; t++) {
        uint64_t before = sums[(size_t)t];
        for (int pass = 0; pass < kDeltaPasses; pass++)
            for (int lane = 0; lane < 64; lane++) {
                uint64_t x[kDeltaUnit];
                int64_t e;
                int cnt;
                const uint64_t mine = delta_decode_load<ES>(jd, t, pass, lane, x, &e, &cnt);
                delta_decode_store<ES>(jd, e, cnt, x, before);
                before += mine;
            }
        for (int lane = 0; lane < 64; lane++) delta_copy_left(jd, t, lane);
    }
    CHECK(memcmp(dec.get(), plain.get(), (size_t)n) == 0, "decode: E %lld es %d flags %d left %d", (long long)E, ES, flags, left);
}

static void test_delta() {
    const int64_t counts[] = {0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, kDeltaTile - 1, kDeltaTile, kDeltaTile + 1, 2 * kDeltaTile + 17};
    for (int64_t E : counts)
        for (int flags = 0; flags < 4; flags++) {
            delta_case<1>(E, 0, flags);
            delta_case<2>(E, flags == 0 ? 1 : 0, flags);
            delta_case<4>(E, flags == 0 ? 3 : 0, flags);
            delta_case<8>(E, flags == 0 ? 7 : 0, flags);
        }
}

// ------------------------------------------------------------------ the byte reversal of place and gather
static void swap_case(int es, int64_t rows, int64_t row, int64_t shape_rows, int64_t shape_row, bool shuffled) {
    ChunkGrid g;
    memset(&g, 0, sizeof g);
    g.rank = 2, g.elem_size = es, g.shape[0] = shape_rows, g.shape[1] = shape_row, g.chunk[0] = rows, g.chunk[1] = row, g.shuffle = shuffled;
    for (int j = 0; j < es; j++) g.fill[j] = (uint8_t)(0xC0 + j);
    int64_t n_chunks, cb, ab;
    CHECK(chunk_grid_check(g, &n_chunks, &cb, &ab), "grid");
    const ChunkGeom geom = chunk_geom(g);
    Block arr(ab), back(ab);
    for (int64_t i = 0; i < ab; i++) arr.get()[i] = rnd();
    memset(back.get(), 0x5A, (size_t)ab);
    const int flags = (shuffled ? 0 : kJobPlain) | kJobSwap;
    for (int64_t c = 0; c < n_chunks; c++) {
        Block chunk(cb), want(cb);
        ChunkJob jb;
        const int64_t origin = chunk_place_of(g, c, jb.ext);
        jb.chunk = chunk.get(), jb.arr = arr.get() + origin * es, jb.geom = 0, jb.flags = flags;
        memset(chunk.get(), 0x5A, (size_t)cb);
        for (int64_t q = 0; q < chunk_item_count(geom, jb.ext, true); q++)
            for (int lane = 0; lane < 64; lane++) chunk_gather_item(geom, jb, q, lane);
        // the model: element (r, k) of the chunk, big-endian, in planes where shuffled
        const int64_t E = rows * row;
        for (int64_t r = 0; r < rows; r++)
            for (int64_t k = 0; k < row; k++)
                for (int j = 0; j < es; j++) {
                    const bool exists = r < jb.ext[0] && k < jb.ext[1];
                    const uint8_t v = exists ? arr.get()[(origin + r * shape_row + k) * es + j] : g.fill[j];
                    const int64_t e = r * row + k;
                    want.get()[shuffled ? (es - 1 - j) * E + e : e * es + (es - 1 - j)] = v;
                }
        CHECK(memcmp(chunk.get(), want.get(), (size_t)cb) == 0, "gather: es %d row %lld chunk %lld shuffled %d", es, (long long)row, (long long)c, (int)shuffled);
        jb.chunk = want.get(), jb.arr = back.get() + origin * es;
        for (int64_t q = 0; q < chunk_item_count(geom, jb.ext, false); q++)
            for (int lane = 0; lane < 64; lane++) chunk_place_item(geom, jb, q, lane);
    }
    CHECK(memcmp(back.get(), arr.get(), (size_t)ab) == 0, "place: es %d row %lld shuffled %d", es, (long long)row, (int)shuffled);
}

static void test_swap() {
    for (int es : {2, 4, 8})
        for (int shuffled = 0; shuffled < 2; shuffled++) {
            swap_case(es, 3, 5, 7, 11, shuffled != 0);      // a lane an element
            swap_case(es, 2, 70, 3, 141, shuffled != 0);    // four elements a lane, a ragged end
            swap_case(es, 2, 600, 3, 1199, shuffled != 0);  // sixteen
            swap_case(es, 2, 608, 2, 1215, shuffled != 0);
        }
}

int main() {
    test_fletcher();
    test_rules();
    test_delta();
    test_swap();
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("PASS chunk filters\n");
    return 0;
}
