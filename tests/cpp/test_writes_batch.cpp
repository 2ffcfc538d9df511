// test_writes_batch.cpp -- the host logic of the batched encoder (no device), with the code the library compiles:
//   zs_core.h write_list_ends / write_block_bytes / layout_write_blocks: what zs_deflate_writes_batch_device makes of the
//     callers' Write lists -- empty Writes dropped, at most one distinct end = one Write, every malformed list rejected, the
//     streams' blocks of the device table 8-byte aligned and disjoint;
//   zs_png.h png_row_image: the image of a flat row, against a linear scan (heights of 1, totals beyond 2^16 rows).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../../zlibstream_amd/csrc/zs_png.h"
using namespace zs;

static int fails = 0;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            if (fails < 20) {                  \
                printf("FAIL %s: ", #c);       \
                printf(__VA_ARGS__);           \
                printf("\n");                  \
            }                                  \
            fails++;                           \
            return;                            \
        }                                      \
    } while (0)

static void check_list(std::mt19937_64 &rng, int id) {
    // a random schedule: sizes of 0 (an empty Write) now and then
    const int nw = (int)(rng() % 40);
    std::vector<int64_t> ends;
    std::vector<int64_t> distinct;
    int64_t at = 0;
    for (int k = 0; k < nw; k++) {
        const int kind = (int)(rng() % 4);
        const int64_t size = kind == 0 ? 0 : kind == 1 ? (int64_t)(rng() % 5) : (int64_t)(rng() % 100000);
        at += size;
        ends.push_back(at);
        if (size > 0) distinct.push_back(at);
    }
    const int64_t n = at;
    std::vector<int64_t> got{-7};
    CHECK(write_list_ends(ends.data(), (int64_t)ends.size(), n, got), "case %d: a well-formed list of %d Writes was rejected", id, nw);
    if (distinct.size() <= 1) CHECK(got.empty(), "case %d: %zu distinct ends must collapse to one Write, got %zu", id, distinct.size(), got.size());
    else CHECK(got == distinct, "case %d: %zu ends, want the %zu distinct ones", id, got.size(), distinct.size());
    for (size_t k = 0; k + 1 < got.size(); k++) CHECK(got[k] < got[k + 1], "case %d: ends not increasing at %zu", id, k);
    if (!got.empty()) CHECK(got.back() == n, "case %d: last end %lld of %lld", id, (long long)got.back(), (long long)n);
    // the malformed variants
    if (!ends.empty()) {
        std::vector<int64_t> bad = ends;
        bad.back() += 1 + (int64_t)(rng() % 3);  // the last end beyond the input
        CHECK(!write_list_ends(bad.data(), (int64_t)bad.size(), n, got), "case %d: a last end beyond the input passed", id);
        if (n > 0) {
            bad = ends;
            bad.back() -= 1;  // the last end short of the input (it may also fall below its predecessor)
            CHECK(!write_list_ends(bad.data(), (int64_t)bad.size(), n, got), "case %d: a last end short of the input passed", id);
        }
        if (ends.size() >= 2) {
            bad = ends;
            const size_t k = (size_t)(rng() % (ends.size() - 1));
            bad[k] = bad[k + 1] + 1 + (int64_t)(rng() % 9);  // an end above its successor
            CHECK(!write_list_ends(bad.data(), (int64_t)bad.size(), n, got), "case %d: decreasing ends passed", id);
        }
        bad = ends;
        bad[(size_t)(rng() % ends.size())] = -1 - (int64_t)(rng() % 5);
        CHECK(!write_list_ends(bad.data(), (int64_t)bad.size(), n, got), "case %d: a negative end passed", id);
    }
    CHECK(write_list_ends(nullptr, 0, 0, got) && got.empty(), "case %d: no Writes and no input is one (empty) Write", id);
    if (n > 0) CHECK(!write_list_ends(nullptr, 0, n, got), "case %d: no Writes for %lld bytes passed", id, (long long)n);
}

static void check_layout(std::mt19937_64 &rng, int id) {
    const int n = 1 + (int)(rng() % 300);
    std::vector<size_t> nw((size_t)n), off;
    for (int i = 0; i < n; i++) nw[(size_t)i] = rng() % 3 == 0 ? 0 : (size_t)(rng() % (rng() % 8 == 0 ? 5000 : 12));
    const size_t total = layout_write_blocks(nw, off);
    CHECK(off.size() == (size_t)n, "case %d: %zu offsets for %d streams", id, off.size(), n);
    size_t end_before = 0;
    for (int i = 0; i < n; i++) {
        CHECK(off[(size_t)i] % 8 == 0, "case %d: stream %d's block at %zu is not 8-byte aligned", id, i, off[(size_t)i]);
        CHECK(off[(size_t)i] >= end_before, "case %d: stream %d's block at %zu overlaps the one before (ends at %zu)", id, i, off[(size_t)i], end_before);
        // [ends: int64][blocks before each Write: int32][flush modes: u8], the three arrays aligned to their types
        const size_t w = nw[(size_t)i], used = 8 * w + 4 * w + w;
        CHECK(write_block_bytes(w) >= used && write_block_bytes(w) < used + 8, "case %d: %zu Writes take %zu bytes", id, w, write_block_bytes(w));
        CHECK((off[(size_t)i] + 8 * w) % 4 == 0, "case %d: stream %d's block counts are not 4-byte aligned", id, i);
        if (w) end_before = off[(size_t)i] + used;
        CHECK(end_before <= total, "case %d: stream %d's block ends at %zu of %zu", id, i, end_before, total);
    }
    CHECK(write_block_bytes(0) == 0, "case %d: a stream without a list takes room", id);
}

static void check_rows(std::mt19937_64 &rng, int id) {
    const int n = 1 + (int)(rng() % (id % 7 == 0 ? 3000 : 40));
    std::vector<int32_t> off((size_t)n + 1, 0);
    for (int i = 0; i < n; i++) {
        const int kind = (int)(rng() % 4);
        const int h = kind == 0 ? 1 : kind == 1 ? 1 + (int)(rng() % 3) : kind == 2 ? 1 + (int)(rng() % 600) : 1 + (int)(rng() % 70000);
        off[(size_t)i + 1] = off[(size_t)i] + h;
    }
    const int64_t total = off[(size_t)n];
    // every row of a small batch; of a large one the rows around every image boundary and a random sample
    auto linear = [&](int64_t r) {
        int i = 0;
        while (off[(size_t)i + 1] <= r) i++;
        return i;
    };
    auto one = [&](int64_t r) {
        const int got = png_row_image(off, n, r), want = n <= 64 ? linear(r) : -1;
        CHECK(got >= 0 && got < n && off[(size_t)got] <= r && r < off[(size_t)got + 1], "case %d: row %lld of %lld -> image %d of %d", id, (long long)r,
              (long long)total, got, n);
        if (want >= 0) CHECK(got == want, "case %d: row %lld -> image %d, the linear scan says %d", id, (long long)r, got, want);
    };
    if (total <= 200000 && n <= 64)
        for (int64_t r = 0; r < total; r++) one(r);
    for (int i = 0; i < n; i++) {
        one(off[(size_t)i]);
        one((int64_t)off[(size_t)i + 1] - 1);
    }
    for (int k = 0; k < 2000; k++) one((int64_t)(rng() % (uint64_t)total));
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 5000;
    std::mt19937_64 rng(20240611);
    int64_t most_rows = 0;
    for (int id = 0; id < cases; id++) {
        check_list(rng, id);
        check_layout(rng, id);
        if (id % 10 == 0) check_rows(rng, id);
    }
    {
        // heights of 1 only, and one batch whose total crosses 2^16 rows by design
        const int n = 70000;
        std::vector<int32_t> off((size_t)n + 1);
        for (int i = 0; i <= n; i++) off[(size_t)i] = i;
        for (int r = 0; r < n; r++)
            if (png_row_image(off, n, r) != r) {
                printf("FAIL: heights of 1: row %d -> image %d\n", r, png_row_image(off, n, r));
                fails++;
                break;
            }
        most_rows = n;
    }
    if (fails) {
        printf("%d failures\n", fails);
        return 1;
    }
    printf("PASS: %d random Write lists, layouts and row lists (up to %lld rows of height 1)\n", cases, (long long)most_rows);
    return 0;
}
