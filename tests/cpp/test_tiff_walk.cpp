// test_tiff_walk.cpp -- the TIFF rules of zlibstream_amd/csrc/zs_tiff.h on the host, built with -fsanitize=address,undefined
// by tests/test_tiff_host.py:
//   - tiff_walk on every file given on the command line (tests/tiff_cases.py builds them: both byte orders, classic and
//     BigTIFF, strips and tiles, two pages) and on every prefix of each, every one in a heap block of exactly its length, so
//     that a read past the end is the sanitizer's to report; a prefix never gives more chunks than the whole file, and a
//     chunk it calls whole lies inside it;
//   - the writer's head read back by the walk;
//   - the predictor kernels' per-lane step (tiff_unpack, tiff_lane_scan, tiff_lane_add, tiff_pack, tiff_phase) over a model
//     of the wave -- 64 lanes of 16-byte groups, passes with a carry per channel, as zs_tiff.hip runs them -- against a scalar
//     loop, for every sample size, 1 .. 8 samples per pixel, both byte orders and rows around a pass's 1024 bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_tiff.h"

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
static int walk_exact(const std::vector<uint8_t> &file, int64_t len, int64_t page, TiffInfo *info, std::vector<TiffChunk> *chunks) {
    uint8_t *block = (uint8_t *)malloc((size_t)len ? (size_t)len : 1);
    memcpy(block, file.data(), (size_t)len);
    int rc = tiff_walk(block, len, page, info, nullptr, 0);
    if (rc == kTiffOk) {
        chunks->assign((size_t)info->n_chunks, TiffChunk{});
        rc = tiff_walk(block, len, page, info, chunks->data(), info->n_chunks);
    }
    free(block);
    return rc;
}

static void test_file(const char *path) {
    const std::vector<uint8_t> file = slurp(path);
    CHECK(!file.empty(), "%s", path);
    TiffInfo whole;
    std::vector<TiffChunk> wc;
    const int rc = walk_exact(file, (int64_t)file.size(), 0, &whole, &wc);
    CHECK(rc == kTiffOk, "%s: %d %s", path, rc, tiff_err_message(rc));
    for (const TiffChunk &c : wc) CHECK(c.status == 0 && c.off + c.comp_len <= (int64_t)file.size() && c.w >= 1 && c.h >= 1, "%s", path);
    for (int64_t page = 0; page < whole.n_pages + 1; page++) {
        for (int64_t len = 0; len <= (int64_t)file.size(); len++) {
            TiffInfo ti;
            std::vector<TiffChunk> ch;
            const int r = walk_exact(file, len, page, &ti, &ch);
            if (len < 8) CHECK(r == kTiffShortFile || r == kTiffBadMagic, "%s cut %lld: %d", path, (long long)len, r);
            if (page >= whole.n_pages && len == (int64_t)file.size()) CHECK(r == kTiffNoPage, "%s page %lld: %d", path, (long long)page, r);
            if (r != kTiffOk) continue;
            CHECK(tiff_err_status(r) == 0 && ti.n_chunks >= 1 && ti.out_len == ti.height * ti.row_bytes, "%s cut %lld", path, (long long)len);
            for (const TiffChunk &c : ch) {
                if (c.status == 0) CHECK(c.off >= 0 && c.comp_len >= 0 && c.off + c.comp_len <= len, "%s cut %lld", path, (long long)len);
                else CHECK(c.status == -5, "%s cut %lld: %d", path, (long long)len, c.status);
                CHECK(c.x + c.w <= ti.width && c.y + c.h <= ti.height, "%s cut %lld", path, (long long)len);
            }
        }
    }
}

// a few headers by hand: each rule of the header and the chain beside a legal file
static void test_headers() {
    TiffInfo ti;
    uint8_t f[64] = {'I', 'I', 42, 0, 8, 0, 0, 0, /* IFD: */ 0, 0, /* next: */ 0, 0, 0, 0};
    CHECK(tiff_walk(f, 14, 0, &ti, nullptr, 0) == kTiffMissingTag && ti.n_pages == 1, "an empty IFD");
    CHECK(tiff_walk(f, 13, 0, &ti, nullptr, 0) == kTiffBadIfd, "an IFD cut in its next pointer");
    CHECK(tiff_walk(f, 7, 0, &ti, nullptr, 0) == kTiffShortFile, "a short header");
    f[2] = 41;
    CHECK(tiff_walk(f, 14, 0, &ti, nullptr, 0) == kTiffBadMagic, "version 41");
    f[2] = 42, f[10] = 8;  // the IFD's next pointer is the IFD itself
    CHECK(tiff_walk(f, 14, 0, &ti, nullptr, 0) == kTiffLoop, "a chain that loops");
    f[10] = 0, f[4] = 4;
    CHECK(tiff_walk(f, 14, 0, &ti, nullptr, 0) == kTiffBadIfd, "an IFD inside the header");
    uint8_t b[40] = {'M', 'M', 0, 43, 0, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 16};
    CHECK(tiff_walk(b, 32, 0, &ti, nullptr, 0) == kTiffMissingTag && ti.bigtiff == 1 && ti.big_endian == 1, "an empty BigTIFF IFD");
    CHECK(tiff_walk(b, 15, 0, &ti, nullptr, 0) == kTiffShortFile, "a short BigTIFF header");
    b[5] = 4;
    CHECK(tiff_walk(b, 32, 0, &ti, nullptr, 0) == kTiffBadMagic, "BigTIFF with 4-byte offsets");
}

// the writer's head, read back
static void test_writer() {
    for (int tiled = 0; tiled < 2; tiled++)
        for (int spp = 1; spp <= 8; spp++)
            for (int extra = 0; extra < spp; extra += 3) {
                TiffLayout l{};
                l.width = 100, l.height = 70, l.bits = 16, l.spp = spp, l.sample_format = 1, l.photometric = spp >= 3 ? 2 : 1;
                l.extra_samples = extra, l.extra_kind = 2, l.predictor = 2, l.tiled = tiled;
                l.chunk_w = tiled ? 32 : 100, l.chunk_h = tiled ? 16 : 30;
                l.across = tiled ? 4 : 1, l.n_chunks = tiled ? 4 * 5 : 3;
                std::vector<int64_t> lens((size_t)l.n_chunks), offs((size_t)l.n_chunks);
                for (size_t k = 0; k < lens.size(); k++) lens[k] = 11 + (int64_t)k;
                const int64_t head = tiff_head_bytes(l);
                std::vector<uint8_t> file((size_t)head);
                const int64_t total = tiff_put_head(file.data(), l, lens.data(), offs.data());
                file.resize((size_t)total, 0);
                TiffInfo ti;
                std::vector<TiffChunk> ch;
                const int rc = walk_exact(file, total, 0, &ti, &ch);
                CHECK(rc == kTiffOk, "writer %d %d: %s", tiled, spp, tiff_err_message(rc));
                CHECK(ti.width == 100 && ti.height == 70 && ti.bits == 16 && ti.spp == spp && ti.predictor == 2 && ti.compression == 8 && ti.tiled == tiled &&
                          ti.n_chunks == l.n_chunks && ti.chunk_w == l.chunk_w && ti.chunk_h == l.chunk_h && ti.extra_samples == extra && ti.n_pages == 1,
                      "writer %d %d", tiled, spp);
                int64_t at = head;
                for (size_t k = 0; k < ch.size(); k++) {
                    CHECK(ch[k].off == at && ch[k].off == offs[k] && ch[k].off % 2 == 0 && ch[k].comp_len == lens[k] && ch[k].status == 0, "writer chunk %zu", k);
                    at += (lens[k] + 1) & ~(int64_t)1;
                }
                CHECK(at == total, "writer total");
            }
}

// ---- the model of the wave
static void load_group(const uint8_t *p, int off, int n, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    for (int b = off; b < n && b < off + 16; b++) w[(b - off) >> 2] |= (uint32_t)p[b] << (8 * ((b - off) & 3));
}
static void store_group(uint8_t *p, int off, int n, const uint32_t w[4]) {
    for (int b = off; b < n && b < off + 16; b++) p[b] = (uint8_t)(w[(b - off) >> 2] >> (8 * ((b - off) & 3)));
}

template <int E, int SPP>
static void wave_pass(uint32_t v[64][E], const int p0[64], uint32_t *carry) {
    uint32_t tot[64][SPP];
    for (int lane = 0; lane < 64; lane++) tiff_lane_scan<E, SPP>(v[lane], p0[lane], tot[lane]);
    for (int c = 0; c < SPP; c++) {
        uint32_t run = carry[c];
        for (int lane = 0; lane < 64; lane++) {
            const uint32_t mine = tot[lane][c];
            tot[lane][c] = run;  // what lies in front of the lane
            run += mine;
        }
        carry[c] = run;
    }
    for (int lane = 0; lane < 64; lane++) tiff_lane_add<E, SPP>(v[lane], p0[lane], tot[lane]);
}

template <int S, int SPP>
static void model_undo_row(const uint8_t *src, uint8_t *dst, int nb, int cb, bool swap) {
    constexpr int E = 16 / S;
    uint32_t carry[SPP] = {};
    for (int base = 0; base < cb; base += 1024) {
        uint32_t v[64][E];
        int p0[64];
        for (int lane = 0; lane < 64; lane++) {
            uint32_t w[4];
            load_group(src, base + 16 * lane, nb, w);
            tiff_unpack<S>(w, v[lane], swap);
            p0[lane] = tiff_phase<E, SPP>((base + 16 * lane) >> 4);
        }
        wave_pass<E, SPP>(v, p0, carry);
        for (int lane = 0; lane < 64; lane++) {
            uint32_t w[4];
            tiff_pack<S>(v[lane], w);
            store_group(dst, base + 16 * lane, cb, w);
        }
    }
}

template <int S, int SPP>
static void test_rows() {
    const int lengths[] = {1, 2, 15, 16, 17, 63, 64, 65, 1008, 1023, 1024, 1025, 2047, 2049, 3100};
    for (int nbytes : lengths)
        for (int swap = 0; swap < (S > 1 ? 2 : 1); swap++) {
            const int ns = (nbytes + S - 1) / S / SPP * SPP + SPP, nb = ns * S;  // whole pixels
            const int cb = nb > 3 * SPP * S ? nb - 2 * SPP * S : nb;             // a clipped part
            std::vector<uint8_t> src((size_t)nb), want((size_t)nb), got((size_t)cb + 1, 0xA5);
            uint32_t seed = (uint32_t)(nbytes * 131 + S * 7 + SPP);
            for (int i = 0; i < nb; i++) seed = seed * 1664525u + 1013904223u, src[(size_t)i] = nbytes % 3 == 0 ? 0xFF : (uint8_t)(seed >> 24);
            // the scalar rule: sample s += sample s - SPP, mod 2^(8 S), read in the file's order, written little-endian
            std::vector<uint32_t> val((size_t)ns);
            for (int s = 0; s < ns; s++) {
                uint32_t x = 0;
                for (int b = 0; b < S; b++) x |= (uint32_t)src[(size_t)(s * S + b)] << (8 * (swap ? S - 1 - b : b));
                val[(size_t)s] = x + (s >= SPP ? val[(size_t)(s - SPP)] : 0);
                for (int b = 0; b < S; b++) want[(size_t)(s * S + b)] = (uint8_t)(val[(size_t)s] >> (8 * b));
            }
            model_undo_row<S, SPP>(src.data(), got.data(), nb, cb, swap != 0);
            CHECK(memcmp(got.data(), want.data(), (size_t)cb) == 0 && got[(size_t)cb] == 0xA5, "S %d SPP %d row %d swap %d", S, SPP, nb, swap);
        }
}

template <int SPP>
static void test_all_sizes() {
    test_rows<1, SPP>();
    test_rows<2, SPP>();
    test_rows<4, SPP>();
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; i++) test_file(argv[i]);
    test_headers();
    test_writer();
    test_all_sizes<1>(), test_all_sizes<2>(), test_all_sizes<3>(), test_all_sizes<4>();
    test_all_sizes<5>(), test_all_sizes<6>(), test_all_sizes<7>(), test_all_sizes<8>();
    if (failures) {
        printf("FAILED: %d checks\n", failures);
        return 1;
    }
    printf("PASS: %d files\n", argc - 1);
    return 0;
}
