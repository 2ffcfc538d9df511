// The schedule of the match kernel's walk (zlibstream_amd/csrc/zs_kernels.hip, match_walk<false>) on the host: 64 lanes in
// lock step, the ballot a 64-bit mask, one position cursor, the stepping phase running until half as many lanes wait as
// step (ZS_WQ : ZS_WD = 2 : 1) with four steps per look at the lane counts, then the compare block, up to four rounds of
// the extension loop and the finish phase once for all waiting lanes.  The same state machine runs with a first compare
// of 8 and of 16 bytes (ZS_CMP16 = 0 / 1).
//
// Asserted, for either width: every position's two records (budgets K and K >> 2) equal zs_core.h's walk_matches over the
// same links, and the loop ends; both widths meet the same candidates, the wider compare never runs more extension rounds,
// and at least halves them where fewer than a tenth of the compares that pass 8 bytes pass 16 (text).  Printed: how often each block of the kernel runs per position, and the wave-instructions
// that makes with the blocks' vector-instruction counts.
//
//   test_match_sched [file ...]     the built-in inputs, then each file (statistics for the files, level 6)
// Prints PASS on its last line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

constexpr int kNone = 0xFFFF;  // the staged form of "no link" (a step over it lands beyond kMaxDist)
constexpr int kPad = 320;      // zero bytes behind the input, as the kernel stages them

// vector instructions of the walk's blocks in the gfx950 code of match_walk<false> (hipcc -O3), per execution by a wave
constexpr double kStepValu = 21, kFinishValu = 58, kCmp8Valu = 43, kCmp16Valu = 58, kRoundValu = 66;

struct Input {
    std::vector<uint8_t> b;  // n bytes + kPad zeros
    std::vector<uint16_t> link;
    int64_t n = 0;
};

// K1's links: link[q] = distance from q to the previous position of q's bucket (hash of bytes q+2 .. q+5), 0 if there is
// none within kMaxDist; positions with q + 5 < n are inserted
static void build_links(Input &in) {
    std::vector<int64_t> head(kHashSize, -1);
    in.link.assign((size_t)in.n + kPad, 0);
    for (int64_t q = 0; q + 5 < in.n; q++) {
        uint32_t v;
        memcpy(&v, &in.b[(size_t)q + 2], 4);
        const uint32_t h = hash_mul(v) & kHashMask;
        const int64_t d = head[h] >= 0 ? q - head[h] : 0;
        in.link[(size_t)q] = (uint16_t)(d > kMaxDist ? 0 : d);
        head[h] = q;
    }
}
static Input make_input(const std::vector<uint8_t> &data) {
    Input in;
    in.n = (int64_t)data.size();
    in.b = data;
    in.b.resize(data.size() + kPad, 0);
    build_links(in);
    return in;
}
// the link as the kernel stages it: none for 0 and for a link onto position 0
static int staged_link(const Input &in, int64_t q) {
    const int d = in.link[(size_t)q];
    return (d == 0 || d == q) ? kNone : d;
}
static uint32_t u32_at(const Input &in, int64_t i) {
    uint32_t v = 0;
    for (int k = 0; k < 4; k++)
        if (i + k >= 0) v |= (uint32_t)in.b[(size_t)(i + k)] << (8 * k);
    return v;
}
static uint64_t u64_at(const Input &in, int64_t i) { return (uint64_t)u32_at(in, i) | ((uint64_t)u32_at(in, i + 4) << 32); }

struct Stats {
    uint64_t positions = 0, with_link = 0, candidates = 0, compares = 0, ge8 = 0, ge16 = 0;
    uint64_t looks = 0, step_blocks = 0, visits = 0, cmp_blocks = 0, finish_blocks = 0, rounds = 0, round_lanes = 0, visit_events = 0;
};

struct Lane {
    int st = 3, best = 2, bdist = 0, n_eval = 0, cl = 0, snapped = 0;
    int64_t p = -1, c = 8;
    uint32_t snap = 0, scan_end = 0, mask = 0, fmask = 0;
    uint32_t sc[4] = {0, 0, 0, 0};
};

// the walk over positions [pbeg, pend); recK / recK4 indexed by position.  Returns false when it did not end.
static bool run_walk(const Input &in, int64_t pbeg, int64_t pend, int K, int nice, int width, std::vector<uint32_t> &recK,
                     std::vector<uint32_t> &recK4, Stats &s) {
    const int K4 = K >> 2;
    Lane L[64];
    int64_t cursor = pbeg;
    auto after_compare = [&](Lane &a, int len) {
        len = len > kMaxMatch ? kMaxMatch : len;
        const bool better = len > a.best;
        const bool freeze = better && a.n_eval >= K4 && !a.snapped;
        if (freeze) a.snap = a.best >= kMinMatch ? pack_match(a.best, a.bdist) : kNoMatch, a.snapped = 1;
        if (better) {
            a.best = len, a.bdist = (int)(a.p - a.c);
            a.scan_end = u32_at(in, a.p + len - 3);
            a.mask = a.fmask = 0xFFFFFFFFu;
        }
        const bool nice_hit = better && len >= nice;
        a.cl = 0;
        a.n_eval++;
        const int64_t nc = a.c - staged_link(in, a.c);
        const bool stop = nice_hit || a.n_eval >= K || a.p - nc >= kMaxDist;
        if (!stop) a.c = nc;
        a.st = stop ? 3 : 1;
    };
    auto ballot = [&](auto pred) {
        uint64_t m = 0;
        for (int i = 0; i < 64; i++)
            if (pred(L[i])) m |= 1ull << i;
        return m;
    };
    // every outer round ends at least one walk or advances a compare, every stepping round counts a candidate: a loose bound
    const uint64_t max_rounds = (uint64_t)(pend - pbeg + 64) * (uint64_t)(K + 64) + 1024;
    uint64_t rounds_run = 0;
    for (;;) {
        if (++rounds_run > max_rounds) return false;
        // ---- finish phase
        for (auto &a : L)
            if (a.st == 3 && a.p >= 0) {
                const uint32_t rec = a.best >= kMinMatch ? pack_match(a.best, a.bdist) : kNoMatch;
                recK[(size_t)a.p] = rec, recK4[(size_t)a.p] = a.snapped ? a.snap : rec;
            }
        for (auto &a : L)
            if (a.st == 3) a.p = -1;
        const uint64_t need = ballot([](const Lane &a) { return a.st == 3; });
        if (need) {
            s.finish_blocks++;
            const int64_t base = cursor;
            cursor += __builtin_popcountll(need);
            for (int i = 0; i < 64; i++) {
                Lane &a = L[i];
                if (a.st != 3) continue;
                const int64_t mine = base + __builtin_popcountll(need & ((1ull << i) - 1ull));
                if (mine >= pend) {
                    a.st = 0;
                    continue;
                }
                s.positions++;
                const int l = staged_link(in, mine);
                const bool has = l != kNone;
                if (!has) recK[(size_t)mine] = recK4[(size_t)mine] = kNoMatch;
                a.p = has ? mine : -1;
                a.c = mine - (has ? l : 0);
                a.st = has ? 1 : 3;
                s.with_link += has;
                a.best = 2, a.bdist = 0, a.n_eval = 0, a.snapped = 0, a.cl = 0;
                for (int k = 0; k < 4; k++) a.sc[k] = u32_at(in, mine + 4 * k);
                a.scan_end = a.sc[0] << 8, a.mask = 0xFFFFFF00u, a.fmask = 0x00FFFFFFu;
            }
        }
        if (!ballot([](const Lane &a) { return a.st != 0; })) break;
        // ---- stepping phase
        for (;;) {
            const int nact = __builtin_popcountll(ballot([](const Lane &a) { return a.st == 1; }));
            const int nwait = __builtin_popcountll(ballot([](const Lane &a) { return a.st >= 2; }));
            s.looks++;
            if (nact == 0 || nwait * 2 >= nact * 1) break;
            if (++rounds_run > max_rounds) return false;
            for (int u = 0; u < 4; u++) {
                s.step_blocks++;
                for (auto &a : L) {
                    if (a.st != 1) continue;
                    s.candidates++;
                    const int l = staged_link(in, a.c);
                    const uint32_t e = u32_at(in, a.c + a.best - 3), f = u32_at(in, a.c);
                    const bool pass = (((e ^ a.scan_end) & a.mask) | ((f ^ a.sc[0]) & a.fmask)) == 0;
                    const int ne = a.n_eval + 1;
                    const int64_t nc = a.c - l;
                    const bool stop = ne >= K || a.p - nc >= kMaxDist;
                    if (!pass) a.n_eval = ne;
                    if (!(pass || stop)) a.c = nc;
                    a.st = pass ? 2 : (stop ? 3 : 1);
                    s.compares += pass;
                }
            }
        }
        // ---- compare phase
        s.visits++;
        s.visit_events += (uint64_t)__builtin_popcountll(ballot([](const Lane &a) { return a.st >= 2; }));
        if (ballot([](const Lane &a) { return a.st == 2 && a.cl == 0; })) {
            s.cmp_blocks++;
            for (auto &a : L) {
                if (!(a.st == 2 && a.cl == 0)) continue;
                const uint64_t xlo = u64_at(in, a.c) ^ ((uint64_t)a.sc[0] | ((uint64_t)a.sc[1] << 32));
                const uint64_t xhi = u64_at(in, a.c + 8) ^ ((uint64_t)a.sc[2] | ((uint64_t)a.sc[3] << 32));
                s.ge8 += xlo == 0;
                s.ge16 += xlo == 0 && xhi == 0;
                if (xlo) after_compare(a, __builtin_ctzll(xlo) >> 3);
                else if (width == 8) a.cl = 8;
                else if (xhi) after_compare(a, 8 + (__builtin_ctzll(xhi) >> 3));
                else a.cl = 16;
            }
        }
        for (int r = 0; r < 4; r++) {
            const uint64_t ext = ballot([](const Lane &a) { return a.st == 2 && a.cl != 0; });
            if (!ext) break;
            s.rounds++;
            s.round_lanes += (uint64_t)__builtin_popcountll(ext);
            for (auto &a : L) {
                if (!(a.st == 2 && a.cl != 0)) continue;
                const uint64_t x = u64_at(in, a.p + a.cl) ^ u64_at(in, a.c + a.cl);
                if (x) {
                    after_compare(a, a.cl + (__builtin_ctzll(x) >> 3));
                } else {
                    a.cl += 8;
                    if (a.cl >= kMaxMatch) after_compare(a, kMaxMatch);
                }
            }
        }
    }
    return true;
}

// the plain per-position chain walk over the same links
static void plain_walk(const Input &in, int64_t pbeg, int64_t pend, const LevelCfg &lv, std::vector<uint32_t> &recK, std::vector<uint32_t> &recK4) {
    auto link = [&](int64_t q) { return (int)in.link[(size_t)q]; };
    auto lcp = [&](int64_t p, int64_t c) {
        int len = 0;
        while (len < kMaxMatch && in.b[(size_t)(p + len)] == in.b[(size_t)(c + len)]) len++;
        return len;
    };
    for (int64_t p = pbeg; p < pend; p++) walk_matches(link, lcp, p, lv, recK[(size_t)p], recK4[(size_t)p]);
}

static void print_stats(const char *name, int width, const Stats &s) {
    const double P = (double)s.positions, V = (double)s.visits;
    const double wi = (kStepValu * (double)s.step_blocks + kFinishValu * (double)s.finish_blocks +
                       (width == 8 ? kCmp8Valu : kCmp16Valu) * (double)s.cmp_blocks + kRoundValu * (double)s.rounds) / P;
    printf("%s cmp%-2d positions %llu candidates/pos %.2f compares/pos %.3f ge8/pos %.3f ge16/pos %.4f events/visit %.1f "
           "rounds/visit %.3f lanes/round %.2f wave-instructions/pos %.2f\n",
           name, width, (unsigned long long)s.positions, (double)s.candidates / P, (double)s.compares / P, (double)s.ge8 / P,
           (double)s.ge16 / P, (double)s.visit_events / V, (double)s.rounds / V, s.rounds ? (double)s.round_lanes / (double)s.rounds : 0.0, wi);
}

// both widths against the plain walk; the statistics of both when `stats`
static void check_input(const char *name, const std::vector<uint8_t> &data, int level, bool stats) {
    const Input in = make_input(data);
    const LevelCfg lv = level_cfg(level);
    const int64_t pbeg = 1, pend = in.n - kMinLookahead + 1;  // the kernel's positions: 1 .. body_end
    if (pend <= pbeg) return;
    std::vector<uint32_t> wantK((size_t)in.n, 0), wantK4((size_t)in.n, 0);
    plain_walk(in, pbeg, pend, lv, wantK, wantK4);
    Stats both[2];
    for (int width = 8; width <= 16; width += 8) {
        std::vector<uint32_t> gotK((size_t)in.n, 0xDEADBEEFu), gotK4((size_t)in.n, 0xDEADBEEFu);
        Stats s;
        const bool ended = run_walk(in, pbeg, pend, lv.chain, lv.nice, width, gotK, gotK4, s);
        CHECK(ended, "%s level %d cmp%d: the walk did not end", name, level, width);
        if (!ended) continue;
        int64_t bad = -1;
        for (int64_t p = pbeg; p < pend && bad < 0; p++)
            if (gotK[(size_t)p] != wantK[(size_t)p] || gotK4[(size_t)p] != wantK4[(size_t)p]) bad = p;
        CHECK(bad < 0, "%s level %d cmp%d: position %lld has %08x / %08x, the plain walk %08x / %08x", name, level, width, (long long)bad,
              gotK[(size_t)bad], gotK4[(size_t)bad], wantK[(size_t)bad], wantK4[(size_t)bad]);
        CHECK(s.positions == (uint64_t)(pend - pbeg), "%s level %d cmp%d: %llu positions handed out of %lld", name, level, width,
              (unsigned long long)s.positions, (long long)(pend - pbeg));
        if (stats) print_stats(name, width, s);
        both[width == 16] = s;
    }
    // a lane's walk does not depend on the width: the same candidates and compares; and what the wider compare is for: on text
    // the extension rounds become rare
    CHECK(both[0].candidates == both[1].candidates && both[0].compares == both[1].compares && both[0].ge8 == both[1].ge8,
          "%s level %d: the two widths walked different candidates", name, level);
    CHECK(both[1].rounds <= both[0].rounds, "%s level %d: %llu extension rounds with 16 bytes, %llu with 8", name, level,
          (unsigned long long)both[1].rounds, (unsigned long long)both[0].rounds);
    if (stats && both[0].ge16 * 10 < both[0].ge8)  // text: few of the compares that pass 8 bytes pass 16
        CHECK(both[1].rounds * 2 < both[0].rounds, "%s level %d: %llu extension rounds with 16 bytes, %llu with 8: not halved", name, level,
              (unsigned long long)both[1].rounds, (unsigned long long)both[0].rounds);
}

// ------------------------------------------------------------------ built-in inputs
static uint32_t rng_state = 12345;
static uint32_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 17, rng_state ^= rng_state << 5;
    return rng_state;
}
static std::vector<uint8_t> word_soup(size_t n, int words) {
    std::vector<std::string> vocab;
    for (int i = 0; i < words; i++) {
        std::string w;
        const int len = 2 + (int)(rnd() % 9);
        for (int k = 0; k < len; k++) w += (char)('a' + rnd() % 26);
        vocab.push_back(w);
    }
    std::vector<uint8_t> out;
    while (out.size() < n) {
        // a skewed choice, so that frequent words repeat in pairs and triples as in prose
        const uint32_t r = rnd() % (uint32_t)words, r2 = rnd() % (uint32_t)words;
        const std::string &w = vocab[r < r2 ? r : r2];
        out.insert(out.end(), w.begin(), w.end());
        out.push_back(' ');
    }
    out.resize(n);
    return out;
}
static std::vector<uint8_t> random_bytes(size_t n, int alphabet) {
    std::vector<uint8_t> out(n);
    for (auto &v : out) v = (uint8_t)(rnd() % (uint32_t)alphabet);
    return out;
}
// random filler with copies of earlier text of exactly `len` bytes (a differing byte behind each copy), two or three per
// source so that chains hold a first candidate, a later better one and ties
static std::vector<uint8_t> exact_matches(size_t n) {
    static const int lens[] = {3, 4, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 257, 258, 300};
    std::vector<uint8_t> out = random_bytes(600, 256);
    while (out.size() < n) {
        const int len = lens[rnd() % (sizeof(lens) / sizeof(lens[0]))];
        const size_t back = 1 + rnd() % (out.size() - 320 < 30000 ? out.size() - 320 : 30000);
        const size_t src = out.size() - back;
        for (int k = 0; k < len; k++) out.push_back(out[src + (size_t)k]);
        out.push_back((uint8_t)(out[src + (size_t)len] ^ (1 + rnd() % 255)));
        const int fill = (int)(rnd() % 24);
        for (int k = 0; k < fill; k++) out.push_back((uint8_t)rnd());
    }
    out.resize(n);
    return out;
}

int main(int argc, char **argv) {
    const int levels[] = {4, 6, 9};
    const std::vector<uint8_t> soup = word_soup(96 * 1024, 900);
    const std::vector<uint8_t> exact = exact_matches(64 * 1024);
    std::vector<uint8_t> periodic(40000), zeros(3000, 0), mixed = word_soup(20000, 60);
    for (size_t i = 0; i < periodic.size(); i++) periodic[i] = (uint8_t)("QRSTUVW"[i % 7]);
    for (size_t i = 0; i < 6000; i++) mixed.push_back((uint8_t)(i % 19 == 0 ? 'x' : 'y'));
    const std::vector<uint8_t> tail = word_soup(4000, 60);
    mixed.insert(mixed.end(), tail.begin(), tail.end());
    for (int level : levels) {
        check_input("soup", soup, level, level == 6);
        check_input("exact", exact, level, false);
        check_input("periodic", periodic, level, false);
        check_input("zeros", zeros, level, false);
        check_input("mixed", mixed, level, false);
        check_input("random4", random_bytes(30000, 4), level, false);
    }
    check_input("short", std::vector<uint8_t>(soup.begin(), soup.begin() + 300), 6, false);
    for (int i = 1; i < argc; i++) {
        FILE *f = fopen(argv[i], "rb");
        CHECK(f != nullptr, "cannot open %s", argv[i]);
        if (!f) continue;
        std::vector<uint8_t> data;
        uint8_t buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + got);
        fclose(f);
        const char *base = strrchr(argv[i], '/');
        check_input(base ? base + 1 : argv[i], data, 6, true);
    }
    printf(fails ? "FAILED %d checks\n" : "PASS\n", fails);
    return fails ? 1 : 0;
}
