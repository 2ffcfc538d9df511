// test_chunk_rows.cpp -- the chunked-array rules of zlibstream_amd/csrc/zs_chunk.h on the host, built with
// -fsanitize=address,undefined by tests/test_chunk_host.py: the decomposition of a flat item index into (chunk, row, stretch)
// and the per-lane steps of the place, gather and survey kernels over a model of the wave -- every item of every chunk, lanes
// 0..63 one after the other -- against a scalar loop over the chunk's coordinates.  Ranks 1..4 with every axis 1 below, on and
// 1 above a chunk multiple, rows that take each lane unit (16, 4 and 1 elements), rows one element short of a whole unit (71 of 72,
// 607 of 608, 527 of 528) and rows of more than one stretch, every elem_size
// 1..16, shuffled and plain chunks, missing and skipped ones.  Every buffer is a heap block of exactly its length, so a byte
// touched outside is the sanitizer's to report; a destination starts as the complement of what is expected, is put back after
// every lane, and so shows every byte that a lane writes: each is written exactly once, with the right value, and nothing
// outside the item's own bytes changes.
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

static uint32_t rng_state = 12345;
static uint8_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 24);
}

struct Block {  // a heap block of exactly n bytes
    std::unique_ptr<uint8_t[]> p;
    int64_t n;
    explicit Block(int64_t len) : p(new uint8_t[(size_t)(len ? len : 1)]), n(len) {}
    uint8_t *get() { return p.get(); }
};

struct Range {
    int64_t lo, hi;
};

// A destination under watch: `want` is what it must hold in the end (`touched[b]`: byte b is to be written at all).
struct Watch {
    uint8_t *buf;
    const uint8_t *want;
    int64_t n;
    std::vector<uint8_t> count;
    Watch(uint8_t *b, const uint8_t *w, int64_t len) : buf(b), want(w), n(len), count((size_t)len, 0) {
        for (int64_t i = 0; i < n; i++) buf[i] = (uint8_t)~want[i];
    }
    // after one lane's call: the bytes of the ranges that changed are counted, checked and put back
    void lane_done(const std::vector<Range> &ranges, const char *what) {
        for (const Range &r : ranges)
            for (int64_t b = r.lo; b < r.hi; b++)
                if (buf[b] != (uint8_t)~want[b]) {
                    CHECK(buf[b] == want[b], "%s: byte %lld is %d, not %d", what, (long long)b, buf[b], want[b]);
                    CHECK(count[(size_t)b] == 0, "%s: byte %lld written twice", what, (long long)b);
                    count[(size_t)b]++;
                    buf[b] = (uint8_t)~want[b];
                }
    }
    // after an item: nothing around its ranges has changed (and in the end nothing anywhere: a byte written outside a range is
    // never put back)
    void item_done(const std::vector<Range> &ranges, const char *what) {
        for (const Range &r : ranges)
            for (int64_t b = r.lo - 32; b < r.hi + 32; b++) {
                if (b < 0 || b >= n || (b >= r.lo && b < r.hi)) continue;
                bool inside = false;
                for (const Range &o : ranges) inside = inside || (b >= o.lo && b < o.hi);
                if (!inside) CHECK(buf[b] == (uint8_t)~want[b], "%s: byte %lld outside the item changed", what, (long long)b);
            }
    }
    void all_done(const std::vector<uint8_t> &touched, const char *what) {
        for (int64_t b = 0; b < n; b++) {
            CHECK(count[(size_t)b] == touched[(size_t)b], "%s: byte %lld written %d times, expected %d", what, (long long)b, count[(size_t)b], touched[(size_t)b]);
            CHECK(buf[b] == (uint8_t)~want[b], "%s: byte %lld was written from outside its item", what, (long long)b);
        }
    }
};

// the scalar rule: chunk element q (C order over chunk[]) of cell p is array element p * chunk + q, where that exists
template <class F>
static void for_each_element(const ChunkGrid &g, int64_t c, F f) {
    int64_t cells[8], p[8];
    for (int d = 0; d < g.rank; d++) cells[d] = (g.shape[d] + g.chunk[d] - 1) / g.chunk[d];
    for (int d = g.rank - 1; d >= 0; d--) p[d] = c % cells[d], c /= cells[d];
    int64_t E = 1;
    for (int d = 0; d < g.rank; d++) E *= g.chunk[d];
    for (int64_t e = 0; e < E; e++) {
        int64_t rest = e, at = 0, stride = 1;
        bool exists = true;
        for (int d = g.rank - 1; d >= 0; d--) {
            const int64_t q = rest % g.chunk[d], idx = p[d] * g.chunk[d] + q;
            rest /= g.chunk[d];
            exists = exists && idx < g.shape[d];
            at += idx * stride, stride *= g.shape[d];
        }
        f(e, exists, at);
    }
}

static void run_grid(const ChunkGrid &g, const char *name) {
    int64_t n_chunks = 0, chunk_bytes = 0, array_bytes = 0;
    CHECK(chunk_grid_check(g, &n_chunks, &chunk_bytes, &array_bytes), "%s: the grid is legal", name);
    const ChunkGeom geom = chunk_geom(g);
    const int es = g.elem_size;
    const int64_t E = chunk_bytes / es;
    CHECK(geom.E == E && geom.unit == chunk_unit(g.chunk[g.rank - 1]) && geom.stretch == 256 * geom.unit, "%s: the geometry", name);
    char what[160];

    // ---- place: chunks of noise; every fourth one plain, every fourth one missing, one in five skipped
    {
        std::vector<Block> chunks;
        Block want(array_bytes), arr(array_bytes);
        std::vector<uint8_t> touched((size_t)array_bytes, 0);
        for (int64_t i = 0; i < array_bytes; i++) want.get()[i] = rnd();  // (what a skipped region keeps: anything)
        std::vector<int> flags((size_t)n_chunks);
        for (int64_t c = 0; c < n_chunks; c++) {
            chunks.emplace_back(chunk_bytes);
            for (int64_t i = 0; i < chunk_bytes; i++) chunks.back().get()[i] = rnd();
            const bool skip = c % 5 == 3;
            flags[(size_t)c] = skip ? -1 : c % 4 == 1 ? (int)kJobPlain : c % 4 == 2 ? (int)kJobFill : 0;
            if (skip) continue;
            const uint8_t *src = chunks.back().get();
            for_each_element(g, c, [&](int64_t e, bool exists, int64_t at) {
                if (!exists) return;
                for (int j = 0; j < es; j++) {
                    want.get()[at * es + j] = flags[(size_t)c] == kJobFill ? g.fill[j] : flags[(size_t)c] == kJobPlain ? src[e * es + j] : src[j * E + e];
                    touched[(size_t)(at * es + j)] = 1;
                }
            });
        }
        Watch w(arr.get(), want.get(), array_bytes);
        for (int64_t c = 0; c < n_chunks; c++) {
            if (flags[(size_t)c] < 0) continue;
            ChunkJob jb;
            const int64_t origin = chunk_place_of(g, c, jb.ext);
            jb.chunk = flags[(size_t)c] == kJobFill ? nullptr : chunks[(size_t)c].get(), jb.arr = arr.get() + origin * es, jb.geom = 0, jb.flags = flags[(size_t)c];
            const int64_t items = chunk_item_count(geom, jb.ext, false);
            for (int64_t q = 0; q < items; q++) {
                const ChunkItem it = chunk_item(geom, jb.ext, false, q);
                CHECK(it.n >= 1 && it.n <= geom.stretch && it.n_exist == it.n, "%s: place item %lld of chunk %lld", name, (long long)q, (long long)c);
                const std::vector<Range> span{{(origin + it.a_off) * es, (origin + it.a_off + it.n) * es}};
                snprintf(what, sizeof what, "%s es %d place chunk %lld item %lld", name, es, (long long)c, (long long)q);
                for (int lane = 0; lane < 64; lane++) {
                    chunk_place_item(geom, jb, q, lane);
                    w.lane_done(span, what);
                }
                w.item_done(span, what);
            }
        }
        w.all_done(touched, name);
    }

    // ---- gather: an array of noise into every chunk, shuffled and plain; the survey on the way
    {
        Block arr(array_bytes);
        for (int64_t i = 0; i < array_bytes; i++) arr.get()[i] = rnd();
        // chunk 0's existing elements are fill, the last chunk's too but for one byte
        std::vector<int64_t> last_chunk_bytes;
        for (int64_t c : {(int64_t)0, n_chunks - 1})
            for_each_element(g, c, [&](int64_t, bool exists, int64_t at) {
                if (!exists) return;
                for (int j = 0; j < es; j++) arr.get()[at * es + j] = g.fill[j];
                if (c == n_chunks - 1) last_chunk_bytes.push_back(at * es + (at % es));
            });
        if (n_chunks > 1) arr.get()[last_chunk_bytes[last_chunk_bytes.size() / 2]] ^= 0x40;
        for (int64_t turn = 0; turn < 2 * n_chunks; turn++) {  // (every chunk both ways: the edge chunks too)
            const int64_t c = turn / 2;
            const bool plain = turn & 1;
            Block want(chunk_bytes), out(chunk_bytes);
            bool all_fill = true;
            for_each_element(g, c, [&](int64_t e, bool exists, int64_t at) {
                for (int j = 0; j < es; j++) {
                    const uint8_t v = exists ? arr.get()[at * es + j] : g.fill[j];
                    want.get()[plain ? e * es + j : j * E + e] = v;
                    all_fill = all_fill && v == g.fill[j];
                }
            });
            Watch w(out.get(), want.get(), chunk_bytes);
            ChunkJob jb;
            const int64_t origin = chunk_place_of(g, c, jb.ext);
            jb.chunk = out.get(), jb.arr = arr.get() + origin * es, jb.geom = 0, jb.flags = plain ? kJobPlain : 0;
            const int64_t items = chunk_item_count(geom, geom.chunk, true);
            CHECK(items == chunk_item_count(geom, jb.ext, true), "%s: the gather's items do not depend on the extent", name);
            for (int64_t q = 0; q < items; q++) {
                const ChunkItem it = chunk_item(geom, jb.ext, true, q);
                std::vector<Range> span;
                if (plain) span.push_back({it.c_off * es, (it.c_off + it.n) * es});
                else
                    for (int j = 0; j < es; j++) span.push_back({j * E + it.c_off, j * E + it.c_off + it.n});
                snprintf(what, sizeof what, "%s es %d gather chunk %lld item %lld", name, es, (long long)c, (long long)q);
                for (int lane = 0; lane < 64; lane++) {
                    chunk_gather_item(geom, jb, q, lane);
                    w.lane_done(span, what);
                }
                w.item_done(span, what);
            }
            w.all_done(std::vector<uint8_t>((size_t)chunk_bytes, 1), name);
            if (plain) continue;
            // the survey: the conjunction over items and lanes
            bool same = true;
            const int64_t s_items = chunk_item_count(geom, jb.ext, false);
            for (int64_t q = 0; q < s_items; q++)
                for (int lane = 0; lane < 64; lane++) same = chunk_survey_item(geom, jb, q, lane) && same;
            CHECK(same == all_fill, "%s es %d: survey of chunk %lld says %d, the scalar loop %d", name, es, (long long)c, same, all_fill);
            if (c == 0) CHECK(same, "%s: chunk 0 is all fill", name);
            if (c == n_chunks - 1 && n_chunks > 1) CHECK(!same, "%s: the last chunk has one byte changed", name);
        }
    }
}

int main() {
    struct Shape {
        int rank;
        int64_t chunk[4];
        bool all_sizes;  // every elem_size 1..16 (the long rows: those with a path of their own, and two generic ones)
    };
    const Shape shapes[] = {
        {1, {24}, true}, {1, {70}, false}, {1, {72}, true}, {1, {608}, false}, {1, {4100}, false},  // lane units 1, 4, 16; two stretches
        {2, {5, 17}, true}, {2, {3, 70}, true}, {2, {2, 528}, false}, {2, {2, 1030}, false},     // (1030: a stretch of unit 16 and a ragged one)
        {3, {3, 4, 9}, true}, {3, {2, 2, 66}, true}, {4, {2, 3, 2, 7}, true}, {4, {2, 1, 2, 64}, true},
    };
    int grids = 0;
    for (const Shape &s : shapes)
        for (int delta = -1; delta <= 1; delta++)
            for (int es = 1; es <= 16; es++) {
                if (!s.all_sizes && !(es == 1 || es == 2 || es == 3 || es == 4 || es == 8 || es == 13 || es == 16)) continue;
                ChunkGrid g;
                memset(&g, 0, sizeof g);
                g.rank = s.rank, g.elem_size = es, g.shuffle = 1;
                char name[96], *at = name;
                at += snprintf(at, 16, "rank %d", s.rank);
                for (int d = 0; d < s.rank; d++) {
                    g.chunk[d] = s.chunk[d], g.shape[d] = 2 * s.chunk[d] + delta;
                    at += snprintf(at, 16, " %lld/%lld", (long long)g.shape[d], (long long)g.chunk[d]);
                }
                for (int j = 0; j < es; j++) g.fill[j] = (uint8_t)(0xA1 + 7 * j);
                run_grid(g, name);
                grids++;
            }
    // a one-element array, and a chunk larger than the array
    for (int es : {1, 4, 7}) {
        ChunkGrid g;
        memset(&g, 0, sizeof g);
        g.rank = 2, g.elem_size = es, g.shuffle = 1, g.shape[0] = g.shape[1] = 1, g.chunk[0] = g.chunk[1] = 1;
        run_grid(g, "one element");
        g.shape[0] = 3, g.shape[1] = 50, g.chunk[0] = 8, g.chunk[1] = 600;
        run_grid(g, "a chunk larger than the array");
        grids += 2;
    }
    // the grid rules from both sides
    {
        ChunkGrid g;
        memset(&g, 0, sizeof g);
        int64_t a, b, c;
        g.rank = 1, g.elem_size = 1, g.shape[0] = g.chunk[0] = 1;
        CHECK(chunk_grid_check(g, &a, &b, &c) && a == 1 && b == 1 && c == 1, "the smallest grid");
        g.rank = 0;
        CHECK(!chunk_grid_check(g, &a, &b, &c), "rank 0");
        g.rank = 9;
        CHECK(!chunk_grid_check(g, &a, &b, &c), "rank 9");
        g.rank = 8, g.elem_size = 2;
        for (int d = 0; d < 8; d++) g.shape[d] = 200, g.chunk[d] = 1;  // 200^8 * 2 = 5.12e18: inside int64
        CHECK(chunk_grid_check(g, &a, &b, &c) && a == 2560000000000000000LL && c == 2 * a, "200^8 elements of 2 bytes");
        g.shape[7] = 800;
        CHECK(!chunk_grid_check(g, &a, &b, &c), "a product that leaves int64");
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("PASS %d grids\n", grids);
    return 0;
}
