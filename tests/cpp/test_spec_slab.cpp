// The pure parts of the speculative walk's provisional symbols (zlibstream_amd/csrc/zs_core.h: spec_slab_stride,
// spec_cut_index, sym_len, spec_first_start / spec_sym_end / spec_sym_top, SpecSlabSink) on the host, against plain loops
// and against what walk_chunk -- the shared chunk walk, chunk_special_prefix included -- tells a symbol sink.
// Prints PASS on its last line.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_core.h"

using namespace zs;

static int fails = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            if (fails++ < 20) printf("FAIL " __VA_ARGS__), printf("\n"); \
        }                                              \
    } while (0)

// the cut by the definition: symbol g of the stream completes a block iff g + 1 is a multiple of kBlockSyms
static int cut_by_loop(uint32_t base, int count) {
    int cut = -1;
    for (int i = 0; i < count; i++)
        if ((base + (uint32_t)i + 1u) % (uint32_t)kBlockSyms == 0) cut = i;
    return cut;
}

static void check_cut(uint32_t base, int count) {
    const int want = cut_by_loop(base, count), got = spec_cut_index(base, count);
    CHECK(want == got, "cut: base %u count %d: %d, the loop says %d", base, count, got, want);
    const bool by_blocks = base / (uint32_t)kBlockSyms != (base + (uint32_t)count) / (uint32_t)kBlockSyms;
    CHECK(by_blocks == (got >= 0), "cut: base %u count %d: %d against the block numbers", base, count, got);
}

// records of a made-up stream for walk_chunk
struct FakeAcc {
    const std::vector<uint32_t> &k, &k4;
    const std::vector<uint8_t> &b;
    const std::vector<uint16_t> &bk, &lk;
    uint32_t mK(int64_t p) const { return k[(size_t)p]; }
    uint32_t mK4(int64_t p) const { return k4[(size_t)p]; }
    uint8_t byte(int64_t p) const { return b[(size_t)p]; }
    uint32_t bucket(int64_t p) const { return bk[(size_t)p]; }
    int link(int64_t p) const { return lk[(size_t)p]; }
    int run1(int64_t p) const { return 2 + (int)(b[(size_t)p] % 7); }
};
struct Told {
    uint32_t sym;
    int64_t end, top;
};
struct RecordingSink {
    std::vector<Told> &v;
    void operator()(int i, uint32_t sym, int64_t end, int64_t top) {
        if ((size_t)i != v.size()) fails++;
        v.push_back({sym, end, top});
    }
};

int main() {
    std::mt19937_64 rng(20240607);
    auto rnd = [&](uint64_t n) { return (uint64_t)(rng() % n); };

    // ---- sym_len
    for (int b = 0; b < 256; b++) CHECK(sym_len((uint32_t)b) == 1, "literal %d", b);
    for (int len = kMinMatch; len <= kMaxMatch; len++)
        for (int dist : {1, 2, 4096, 32506, 32768})
            CHECK(sym_len(((uint32_t)dist << 16) | (uint32_t)(len - 3)) == len, "match %d / %d", len, dist);

    // ---- the slab: the most a chunk of L positions emits is L symbols (every step one position and one literal), the count
    // field of a record has 12 bits, and the odd-symbol word behind the symbols is the slab's own
    for (int bits : {9, 10, 11}) {
        const int L = 1 << bits, stride = spec_slab_stride(bits);
        CHECK(stride >= L + 1, "stride %d of chunk %d", stride, L);
        CHECK(L <= 0xFFF, "count field, chunk %d", L);
        CHECK(L < kBlockSyms, "one cut per chunk at most, chunk %d", L);
    }

    // ---- the cut: at index 0, at the last index, none, base + count exactly on a multiple, count 0, and at random
    const uint32_t B = (uint32_t)kBlockSyms;
    for (uint32_t blk : {1u, 2u, 7u, 1000u, 262000u}) {
        for (int count : {0, 1, 2, 63, 64, 65, 511, 512, 1024, 2048}) {
            check_cut(blk * B - 1, count);                      // the cut symbol is the slab's first
            if (count) check_cut(blk * B - (uint32_t)count, count);  // ... its last: base + count is a multiple
            check_cut(blk * B, count);                          // the block before ended with the chunk before: none
            check_cut(blk * B - (uint32_t)count - 1, count);    // one short of the cut: none
            check_cut(blk * B + 1, count);
        }
        CHECK(spec_cut_index(blk * B - 1, 5) == 0 && spec_cut_index(blk * B - 5, 5) == 4 && spec_cut_index(blk * B - 6, 5) == -1 &&
                  spec_cut_index(blk * B, 5) == -1,
              "the named cases at block %u", blk);
    }
    check_cut(0, 0), check_cut(0, 2048), check_cut(B - 2048, 2048), check_cut(B - 2047, 2048);
    for (int it = 0; it < 200000; it++) check_cut((uint32_t)rnd(1u << 28), (int)rnd(2049));
    for (int it = 0; it < 200000; it++) {  // near a cut, where the cases are
        const uint32_t blk = 1 + (uint32_t)rnd(16000);
        check_cut(blk * B - (uint32_t)rnd(2100), (int)rnd(2049));
    }

    // ---- position from lengths, against a plain loop over random symbol sequences
    for (int it = 0; it < 20000; it++) {
        const int n = 1 + (int)rnd(2048), slot = (int)rnd(kSlots);
        const int64_t cs = 1024 * (int64_t)rnd(60000) + 763;
        std::vector<uint32_t> syms((size_t)n);
        for (auto &v : syms) v = rnd(3) ? (uint32_t)rnd(256) : ((uint32_t)(1 + rnd(32768)) << 16) | (uint32_t)rnd(256);
        int64_t at = slot <= 256 ? cs + slot : cs - 1;
        CHECK(spec_first_start(cs, slot) == at, "first start, slot %d", slot);
        const int i = (int)rnd((uint64_t)n);
        int64_t before = 0;
        for (int k = 0; k < i; k++) before += (syms[(size_t)k] >> 16) ? (int)(syms[(size_t)k] & 0xFFFF) + 3 : 1;
        int sum = 0;
        for (int k = 0; k < i; k++) sum += sym_len(syms[(size_t)k]);
        CHECK(sum == before, "lengths");
        const int64_t start = at + before;
        const bool lit = syms[(size_t)i] < 256;
        CHECK(spec_sym_end(start, syms[(size_t)i]) == (lit ? start + 1 : start + (int)(syms[(size_t)i] & 0xFFFF) + 3), "end");
        CHECK(spec_sym_top(start, false) == start + 1 && spec_sym_top(start, true) == start + 2, "top");
    }

    // ---- what a sink is told by the shared chunk walk: every symbol's end and loop-top are those that follow from the entry
    // and the lengths in front of it -- plain chunks from every entry slot, and first chunks of segments with a cluster of
    // read boundaries, the slide threshold placed where loop-tops land on it (the odd loop-top)
    int64_t n_syms = 0, n_odd = 0, n_event_chunks = 0;
    int most[kSpecMaxLenBits + 1] = {};  // per chunk length: the most symbols a chunk emitted
    const size_t kN = (size_t)2048 * 80;
    std::vector<uint32_t> k(kN), k4(kN);
    std::vector<uint8_t> b(kN);
    std::vector<uint16_t> bk(kN), lk(kN);
    for (int it = 0; it < 6000; it++) {
        const int bits = 9 + (int)rnd(3), L = 1 << bits;
        const int64_t cs = (int64_t)L * (8 + (int64_t)rnd(64)) - (kMinLookahead - 1), ce = cs + L;
        const int density = (int)rnd(5);  // 0: no matches at all -- the chunk of literals, the largest count
        for (size_t p = (size_t)cs - 8; p < (size_t)ce + 1024; p++) {  // (what a walk of [cs, ce) can read)
            b[p] = (uint8_t)rnd(256), bk[p] = (uint16_t)rnd(4), lk[p] = (uint16_t)(rnd(8) ? rnd(32507) : kMaxDist);
            k[p] = density && rnd(5) < (uint64_t)density ? pack_match(3 + (int)rnd(rnd(4) ? 12 : 256), 1 + (int)rnd(4000)) : kNoMatch;
            k4[p] = rnd(3) ? k[p] : kNoMatch;
        }
        FakeAcc acc{k, k4, b, bk, lk};
        ChunkCtx cx;
        cx.cs = cs, cx.ce = ce, cx.cl = nullptr, cx.m = 0, cx.S = 0, cx.after = 0;
        uint32_t cl[3];
        const bool events = it % 2 == 1;
        if (events) {
            // boundaries read at the first loop-tops at or behind cs + 3 and a little later; the window slides at the first
            n_event_chunks++;
            cl[0] = (uint32_t)(cs + 3 + (kMinLookahead - 1)) | kClWindowBit;
            cl[1] = (uint32_t)(cs + 3 + (kMinLookahead - 1) + 20 + (int)rnd(300));
            cx.cl = cl, cx.m = 1 + (int)rnd(2), cx.S = cs + 3 + (int64_t)rnd(4), cx.after = ce + 100000;
        }
        const LevelCfg lv = level_cfg(4 + (int)rnd(6));
        const int slot = density == 0 ? 257 : (int)rnd(kSlots);
        // an entry with something pending: the record in front of the chunk is what that state says it is
        if (slot == 257) k[(size_t)cs - 1] = k4[(size_t)cs - 1] = kNoMatch;
        if (slot >= 258 && k[(size_t)cs - 1] == kNoMatch) k[(size_t)cs - 1] = pack_match(3 + (int)rnd(256), 1 + (int)rnd(4000));
        if (slot == 259) k4[(size_t)cs - 1] = k[(size_t)cs - 1];
        std::vector<Told> told;
        RecordingSink rs{told};
        int ex, cnt;
        walk_chunk(acc, rs, cx, slot, lv, kDefault, ex, cnt);
        CHECK(cnt == (int)told.size() && cnt <= L, "chunk of %d positions: %d symbols", L, cnt);
        most[bits] = cnt > most[bits] ? cnt : most[bits];
        // the same walk into a slab
        std::vector<uint32_t> slab((size_t)spec_slab_stride(bits), 0xDEADBEEFu);
        SpecSlabSink ss{slab.data(), -1};
        int ex2, cnt2;
        walk_chunk(acc, ss, cx, slot, lv, kDefault, ex2, cnt2);
        CHECK(ex2 == ex && cnt2 == cnt, "the two sinks");
        int64_t start = spec_first_start(cs, slot);
        int odd_seen = -1;
        for (int i = 0; i < cnt; i++) {
            CHECK(slab[(size_t)i] == told[(size_t)i].sym, "symbol %d", i);
            const bool odd = i == ss.odd;
            CHECK(spec_sym_end(start, told[(size_t)i].sym) == told[(size_t)i].end, "end of symbol %d (slot %d, events %d): %lld, told %lld", i, slot,
                  (int)events, (long long)spec_sym_end(start, told[(size_t)i].sym), (long long)told[(size_t)i].end);
            CHECK(spec_sym_top(start, odd) == told[(size_t)i].top, "loop-top of symbol %d (slot %d, events %d)", i, slot, (int)events);
            if (told[(size_t)i].top != start + 1) odd_seen = i;
            start += sym_len(told[(size_t)i].sym);
        }
        CHECK(odd_seen == ss.odd, "the odd symbol: %d, sink says %d", odd_seen, ss.odd);
        CHECK(events || ss.odd < 0, "an odd loop-top in a plain chunk");
        for (size_t i = (size_t)cnt; i < slab.size(); i++) CHECK(slab[i] == 0xDEADBEEFu, "a word behind the symbols was written");
        n_syms += cnt, n_odd += ss.odd >= 0;
    }
    for (int bits : {9, 10, 11})  // the slab holds the largest count of every chunk length, and that count is reached
        CHECK(most[bits] == (1 << bits) && most[bits] <= spec_slab_stride(bits) - 1, "chunks of %d positions: most symbols %d", 1 << bits, most[bits]);
    CHECK(n_odd >= 20, "the odd loop-top was met %lld times only", (long long)n_odd);
    printf("%lld symbols of %d chunks checked, %lld chunks with an odd loop-top of %lld with events, most symbols in a chunk of 512 / 1024 / 2048: %d / %d / %d\n",
           (long long)n_syms, 6000, (long long)n_odd, (long long)n_event_chunks, most[9], most[10], most[11]);
    if (fails) {
        printf("%d check(s) failed\n", fails);
        return 1;
    }
    printf("PASS\n");
    return 0;
}
