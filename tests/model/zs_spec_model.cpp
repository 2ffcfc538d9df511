// zs_spec_model.cpp -- CPU model of the speculative chunk walk (TEST TOOL).
//
// Levels 4-9, one Write: instead of building every chunk's transfer map, each chunk of a grid of its own (chunk j >= 1 begins
// at j * len - 261) is walked from a *guessed* entry -- the node its lazy parse stands in at the first loop-top at or behind
// the chunk's start when it is begun `warm` positions earlier in state R with nothing pending -- and the guesses are checked
// against the exits: chunk 0 starts in the true state, so if every chunk's guess is its predecessor's exit, every walk was the
// true one.  A chunk whose path meets an event that shares its bucket with the next position (a chain is cut: K4's business),
// or a poisoned read, makes the stream bail.  Same ZS_HD code as the kernels (zs_core.h); checked against the oracle's symbol,
// block and read trace.
//
// usage: zs_spec_model <file> <level> <strategy> <len[,len...]> <warm> [corrupt]   -> per length: PASS ... path=spec|maps
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../oracle/zs_oracle.h"
#include "../../zlibstream_amd/csrc/zs_core.h"

using namespace zs;

struct Trace {
    std::vector<uint32_t> syms;
    struct Blk {
        int nsyms;
        int64_t start;
        int stored_len;
    };
    std::vector<Blk> blocks;
    std::vector<int64_t> reads;
};
static void on_symbol(void *u, int dist, int lc, int64_t) { ((Trace *)u)->syms.push_back(((uint32_t)dist << 16) | (uint32_t)lc); }
static void on_block(void *u, int, int nsyms, int64_t start, int stored_len, int, int64_t) { ((Trace *)u)->blocks.push_back({nsyms, start, stored_len}); }
static void on_read(void *u, int64_t s, int, int, int64_t) { ((Trace *)u)->reads.push_back(s); }

struct Model {
    const uint8_t *data;
    int64_t n, body_end;
    int strategy;
    LevelCfg lv;
    std::vector<uint32_t> crc_tab, mK, mK4;
    std::vector<uint16_t> link;
    Geometry geo;
    uint32_t bucket(int64_t p) const {
        uint32_t v = (uint32_t)data[p + 2] | ((uint32_t)data[p + 3] << 8) | ((uint32_t)data[p + 4] << 16) | ((uint32_t)data[p + 5] << 24);
        return crc32c_u32_tab(crc_tab.data(), v) & kHashMask;
    }
    int lcp(int64_t p, int64_t c) const {
        int len = 0;
        while (len < kMaxMatch && data[p + len] == data[c + len]) len++;
        return len;
    }
    void prepare() {
        link.assign((size_t)n + 8, 0);
        std::vector<int64_t> head(kHashSize, -1);
        for (int64_t p = 0; p + 5 < n; p++) {
            const uint32_t h = bucket(p);
            const int64_t c = head[h];
            link[(size_t)p] = (c >= 0 && p - c <= 32767) ? (uint16_t)(p - c) : 0;
            head[h] = p;
        }
        mK.assign((size_t)n + 8, 0), mK4.assign((size_t)n + 8, 0);
        auto lk = [this](int64_t q) { return (int)link[(size_t)q]; };
        auto lc = [this](int64_t a, int64_t c) { return lcp(a, c); };
        for (int64_t p = 1; p <= body_end; p++) walk_matches(lk, lc, p, lv, mK[(size_t)p], mK4[(size_t)p]);
    }
    uint32_t flt(uint32_t m) const { return m ? filter_match(match_len(m), match_dist(m), strategy) : kNoMatch; }
};
struct Acc {
    const Model *m;
    uint32_t mK(int64_t p) const { return m->flt(m->mK[(size_t)p]); }
    uint32_t mK4(int64_t p) const { return m->flt(m->mK4[(size_t)p]); }
    uint8_t byte(int64_t p) const { return m->data[p]; }
    uint32_t bucket(int64_t p) const { return m->bucket(p); }
    int run1(int64_t p) const { return m->lcp(p, p - 1); }
    int link(int64_t p) const { return (int)m->link[(size_t)p]; }
};

// chunk j of the speculative grid (the kernels' spec_chunk_ctx): the segments of a single Write begin at 65275 + 32768 k
static ChunkCtx spec_ctx(const Model &m, int j, int len) {
    ChunkCtx cx;
    cx.cs = j ? (int64_t)j * len - (kMinLookahead - 1) : 0;
    cx.ce = (int64_t)(j + 1) * len - (kMinLookahead - 1);
    if (cx.ce > m.body_end + 1) cx.ce = m.body_end + 1;
    cx.cl = nullptr, cx.m = 0, cx.S = 0, cx.after = 0;
    const int64_t seg1 = kWindowSize - (kMinLookahead - 1);
    if (cx.cs >= seg1 && (cx.cs - seg1) % kWSize == 0) {
        const int k = (int)((cx.cs - seg1) / kWSize) + 1;
        if (k < m.geo.nsegs()) {
            cx.cl = m.geo.cl.data() + m.geo.seg_cl[(size_t)k], cx.m = m.geo.seg_cl[(size_t)k + 1] - m.geo.seg_cl[(size_t)k];
            cx.S = m.geo.seg_S[(size_t)k], cx.after = m.geo.seg_after[(size_t)k];
        }
    }
    return cx;
}

struct SymSink {  // the symbol kernel's sink: symbols in place, the cut of every block that ends in the chunk
    uint32_t base;
    std::vector<uint32_t> *syms;
    std::vector<int64_t> *blk_end, *blk_top;
    void operator()(int i, uint32_t sym, int64_t end, int64_t top) {
        const size_t idx = (size_t)base + (size_t)i;
        (*syms)[idx] = sym;
        if ((idx + 1) % kBlockSyms == 0) (*blk_end)[idx / kBlockSyms] = end, (*blk_top)[idx / kBlockSyms] = top;
    }
};
struct LastEv {
    int64_t pos;
    void operator()(int64_t q, bool) { pos = q; }
};

int main(int argc, char **argv) {
    if (argc < 6) {
        fprintf(stderr, "usage: %s file level strategy len warm [corrupt]\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> buf;
    {
        uint8_t tmp[65536];
        size_t r;
        while ((r = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + r);
        fclose(f);
    }
    const int level = atoi(argv[2]), strategy = atoi(argv[3]), warm = atoi(argv[5]);
    const int corrupt = argc > 6 ? atoi(argv[6]) : -1;
    std::vector<int> lens;  // "512,1024,2048": the chunk lengths to try (the match records are made once)
    for (const char *q = argv[4]; q && *q; q = strchr(q, ',') ? strchr(q, ',') + 1 : nullptr) lens.push_back(atoi(q));
    for (int len : lens)
        if (len != 512 && len != 1024 && len != 2048) return 2;
    if (lens.empty() || warm < 0) return 2;
    const int64_t n = (int64_t)buf.size();
    buf.resize(buf.size() + 1024, 0);

    Trace tr;
    zso_trace t;
    memset(&t, 0, sizeof t);
    t.on_symbol = on_symbol, t.on_block = on_block, t.on_read = on_read, t.user = &tr;
    std::vector<uint8_t> ref(zso_compress_bound((size_t)n) + 64);
    if (zso_compress_stream(buf.data(), (size_t)n, nullptr, 0, level, strategy, 0, 0, ref.data(), ref.size(), &t) == (size_t)-1) {
        printf("oracle failed\n");
        return 1;
    }

    Model m;
    m.data = buf.data(), m.n = n, m.strategy = strategy, m.lv = level_cfg(level);
    m.crc_tab.resize(1024);
    for (int tt = 0; tt < 4; tt++)
        for (int i = 0; i < 256; i++) m.crc_tab[(size_t)tt * 256 + i] = crc32c_table_entry(tt, (uint32_t)i);
    const std::vector<int64_t> no_ends;
    if (m.lv.func != 2 || (strategy != kDefault && strategy != kFiltered) || !build_geometry(n, no_ends, m.geo)) {
        printf("PASS n=%ld level=%d path=none (the stream does not qualify)\n", (long)n, level);
        return 0;
    }
    m.body_end = m.geo.body_end;
    m.prepare();
    Acc acc{&m};
    NullSink nsk;
    bool all_ok = true;
    for (int len : lens) {
    // ---- 1. the walk from guessed entries: guess, exit, count, bail per chunk ----
    const int nsc = (int)((m.body_end + kMinLookahead - 1) / len) + 1;
    std::vector<int> guess((size_t)nsc), exit_slot((size_t)nsc), count((size_t)nsc);
    bool bail = false;
    for (int j = 0; j < nsc; j++) {
        const ChunkCtx cx = spec_ctx(m, j, len);
        int kind = kR;
        int64_t p = j == 0 || cx.cs - warm < 0 ? 0 : cx.cs - warm;
        uint32_t pend = 0;
        while (p < cx.cs) {  // the warm-up: plain steps, nothing emitted, events ignored (a wrong guess is found out below)
            const uint32_t cK = p ? acc.mK(p) : 0, cK4 = p ? acc.mK4(p) : 0;
            const Step st = lazy_step(kind, p, pend, cK, cK4, m.lv);
            pend = st.kind == kXK ? cK : st.kind == kXK4 ? cK4 : 0;
            kind = st.kind, p = st.pos;
        }
        int g = kind == kR ? (int)(p - cx.cs) : 256 + kind;
        if (g < 0 || g >= kSlots || (g > 256 && p != cx.cs)) {
            printf("FAIL chunk %d: the warm-up ends in a node that is no entry slot (kind %d at %ld, chunk from %ld)\n", j, kind, (long)p, (long)cx.cs);
            return 1;  // (cannot happen: a step from below cs lands on cs in L / XK / XK4, or behind a match of at most 258)
        }
        uint32_t flags = 0;
        int ex, cnt;
        walk_chunk(acc, nsk, cx, g, m.lv, strategy, ex, cnt, &flags);
        if (flags & (kMapEqualBit | kMapPoisonBit)) bail = true;
        guess[(size_t)j] = j == corrupt ? (g + 1) % kSlots : g, exit_slot[(size_t)j] = ex, count[(size_t)j] = cnt;
    }
    // ---- 2. verify + scan ----
    int wrong = guess[0] != 0;  // (chunk 0's entry is the stream's initial state, slot 0: the induction's base is checked too)
    for (int j = 1; j < nsc; j++) wrong += guess[(size_t)j] != exit_slot[(size_t)j - 1];
    if (bail || wrong) {
        // the stream is the maps' (tests/model/zs_model.cpp mode chunk is their model): nothing of this walk is used
        printf("PASS n=%ld level=%d strat=%d len=%d warm=%d path=maps chunks=%d wrong=%d bail=%d\n", (long)n, level, strategy, len, warm, nsc, wrong, (int)bail);
        continue;
    }
    std::vector<uint32_t> base((size_t)nsc + 1, 0);
    for (int j = 0; j < nsc; j++) base[(size_t)j + 1] = base[(size_t)j] + (uint32_t)count[(size_t)j];
    const uint32_t body_syms = base[(size_t)nsc];
    // ---- 3. the symbols from the verified entries, in place ----
    std::vector<uint32_t> syms((size_t)body_syms + 1, 0);
    std::vector<int64_t> blk_end(body_syms / kBlockSyms + 1, -1), blk_top(body_syms / kBlockSyms + 1, -1);
    for (int j = 0; j < nsc; j++) {
        SymSink sink{base[(size_t)j], &syms, &blk_end, &blk_top};
        int ex, cnt;
        walk_chunk(acc, sink, spec_ctx(m, j, len), guess[(size_t)j], m.lv, strategy, ex, cnt);
    }
    // what the resolve kernel leaves for the tail engine
    const int last = exit_slot[(size_t)nsc - 1];
    const int64_t tail_p = last <= 256 ? m.body_end + 1 + last : m.body_end + 1;
    int k_done = 0;
    int64_t preins = -1;
    for (int k = m.geo.nsegs() - 1; k >= 1; k--) {
        const int j = (int)(((int64_t)kWindowSize + (int64_t)kWSize * (k - 1)) / len);
        if (j >= nsc) continue;
        const ChunkCtx cx = spec_ctx(m, j, len);
        const int g = guess[(size_t)j];
        if ((g <= 256 ? cx.cs + g : cx.cs) > m.body_end) continue;
        LastEv lev{-1};
        int k2, n2;
        int64_t p2;
        uint32_t f2;
        chunk_special_prefix(acc, nsk, cx, g, m.lv, strategy, k2, p2, n2, f2, lev);
        k_done = k, preins = lev.pos >= 0 ? lev.pos + 1 : -1;
        break;
    }

    // ---- against the oracle ----
    bool ok = true;
    if (body_syms > tr.syms.size()) printf("more body symbols (%u) than the oracle has (%zu)\n", body_syms, tr.syms.size()), ok = false;
    for (size_t i = 0; ok && i < body_syms; i++)
        if (syms[i] != tr.syms[i]) printf("symbol %zu differs: model %08x oracle %08x\n", i, syms[i], tr.syms[i]), ok = false;
    // the oracle's next symbol is the tail engine's: it is emitted at a loop-top behind the body
    for (size_t b = 0; ok && b < body_syms / kBlockSyms; b++) {
        if (b >= tr.blocks.size() || tr.blocks[b].nsyms != kBlockSyms || blk_end[b] != tr.blocks[b].start + tr.blocks[b].stored_len) {
            printf("block %zu: ends at %ld, oracle %ld\n", b, (long)blk_end[b], b < tr.blocks.size() ? (long)(tr.blocks[b].start + tr.blocks[b].stored_len) : -1L);
            ok = false;
        }
        // the loop-top reported with a block's last symbol, by walk_chunk's specification and the oracle's own symbol: a literal is
        // emitted at loop-top p for position p - 1 (end = p), a match of length len at p for the match at p - 1 (end = p - 1 + len);
        // the nil_edge case (top = p + 1) belongs to Write-end events and cannot occur in a single Write
        if (b < tr.blocks.size()) {
            const uint32_t last_sym = tr.syms[(b + 1) * (size_t)kBlockSyms - 1];
            const int64_t want_top = (last_sym >> 16) ? blk_end[b] + 1 - ((int64_t)(last_sym & 0xFFFF) + 3) : blk_end[b];
            if (blk_top[b] != want_top)
                printf("block %zu: last loop-top %ld, expected %ld (end %ld)\n", b, (long)blk_top[b], (long)want_top, (long)blk_end[b]), ok = false;
        }
    }
    {
        // read events that fired in the body: the oracle's reads at loop-tops 0 < r <= body_end (several reads at one loop-top are one)
        int want_k = 0;
        int64_t want_pre = -1, prev = -1;
        for (int64_t r : tr.reads)
            if (r > 0 && r <= m.body_end && r != prev) want_k++, want_pre = r + 1, prev = r;
        if (k_done != want_k || preins != want_pre)
            printf("events: %d fired, pre-insert %ld; oracle %d, %ld\n", k_done, (long)preins, want_k, (long)want_pre), ok = false;
    }
    if (tail_p <= m.body_end || tail_p > m.body_end + 257) printf("tail from %ld, body ends at %ld\n", (long)tail_p, (long)m.body_end), ok = false;
    printf("%s n=%ld level=%d strat=%d len=%d warm=%d path=spec chunks=%d syms=%u blocks=%u events=%d tail_from=%ld\n", ok ? "PASS" : "FAIL", (long)n, level, strategy,
           len, warm, nsc, body_syms, body_syms / kBlockSyms, k_done, (long)tail_p);
    all_ok = all_ok && ok;
    }
    return all_ok ? 0 : 1;
}
