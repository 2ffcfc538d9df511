// The planner of a deflate call (zlibstream_amd/csrc/zs_plan.h) on the host: equal keys give equal plans, every switch the
// planner takes from PlanEnv changes some plan, and on every edge shape the offsets, work lists, table sizes and the staged,
// bound descriptors are what the layout says.  The planner is compiled with getenv poisoned: it cannot read a switch that is
// not in the key.  Stand-alone: g++ -fsanitize=address,undefined tests/cpp/test_plan.cpp && ./a.out
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_plan_key.h"
#pragma GCC poison getenv
#include "../../zlibstream_amd/csrc/zs_plan.h"

using namespace zs;

namespace {
int failures = 0, checks = 0;
void expect(bool ok, const std::string &what) {
    checks++;
    if (!ok) failures++, printf("FAIL: %s\n", what.c_str());
}

// The arguments of a call: the smallest at which a rule of the planner can go wrong.
struct Shape {
    std::string name;
    int level = 6, strategy = kDefault, force_seq = 0;
    std::vector<int64_t> len;
    std::vector<WriteSpec> ws;  // empty: no Write lists; else one per stream, a list without ends meaning "none"
    bool incremental = false;
    PlanRun ro;
    std::string want_err;  // the planner refuses the shape with this
};
WriteSpec writes_of(int64_t len, int64_t step, uint8_t last_flush = 0, uint8_t every_flush = 0) {
    WriteSpec w;
    for (int64_t e = step; e < len; e += step) w.ends.push_back(e), w.flush.push_back(every_flush);
    w.ends.push_back(len), w.flush.push_back(last_flush ? last_flush : every_flush);
    return w;
}
WriteSpec ends_of(std::vector<int64_t> ends) {
    WriteSpec w;
    w.ends = ends, w.flush.assign(ends.size(), 0);
    return w;
}
Shape one(const char *name, int64_t len, int level, int strategy = kDefault) {
    Shape s;
    s.name = name, s.level = level, s.strategy = strategy, s.len = {len};
    return s;
}
std::vector<Shape> edge_shapes() {
    std::vector<Shape> v;
    for (int64_t len : {0, 1, 261, 262, 263, 523, 524, 65274, 65536, 65537})  // (523 / 524: the bulk parse wants 262 loop-tops)
        for (int level : {1, 6}) v.push_back(one(("length " + std::to_string(len) + " at level " + std::to_string(level)).c_str(), len, level));
    v.push_back(one("1 MiB - 1 at level 6 (below the walk)", (1 << 20) - 1, 6));
    v.push_back(one("walk", 1 << 20, 6));
    v.push_back(one("maps", 70000, 6));
    v.push_back(one("level 0", 100000, 0));
    {
        Shape s = one("level 0, flushing Writes", 100000, 0);
        s.ws = {writes_of(100000, 30000, 0, 2)};
        v.push_back(s);
        s = one("level 0, Writes without a flush", 100000, 0);
        s.ws = {writes_of(100000, 30000)};
        v.push_back(s);
    }
    v.push_back(one("rle", 70000, 6, kRle));
    {
        Shape s = one("rle writes", 70000, 6, kRle);  // (Write ends away from the window ends: the single Write's stream)
        s.ws = {ends_of({30000, 70000})};
        v.push_back(s);
        s = one("rle, a Write end 100 bytes below a window end", 140000, 6, kRle);
        s.ws = {ends_of({98304 - 100, 140000})};
        v.push_back(s);
        s = one("rle, a Write end 300 bytes below a window end", 140000, 6, kRle);
        s.ws = {ends_of({98304 - 300, 140000})};
        v.push_back(s);
    }
    v.push_back(one("sweeps", 300000, 1));
    {
        Shape s = one("copyto", 300000, 1);  // Stream.CopyTo's Writes
        s.ws = {writes_of(300000, 81920)};
        v.push_back(s);
        s = one("level 1, Writes of 5 bytes", 3000, 1);
        s.ws = {writes_of(3000, 5)};
        v.push_back(s);
        s = one("level 6, Writes of 5 bytes", 3000, 6);
        s.ws = {writes_of(3000, 5)};
        v.push_back(s);
        s = one("dual", 300000, 1);
        s.len = {300000, 300000, 300000, 300000};
        v.push_back(s);
        s.name = "dual struck", s.len[2] = 100;
        v.push_back(s);
        s = one("64 streams", 40000, 6);
        s.len.assign(64, 40000);
        v.push_back(s);
        s.name = "65 streams", s.len.assign(65, 40000), s.len[7] = 65537, s.len[64] = 0;
        v.push_back(s);
        s = one("one long stream among 5000 short ones", 100, 6);
        s.len.assign(5001, 100), s.len[2500] = 3 << 20;
        v.push_back(s);
        s = one("a batch with a Write list for one stream", 70000, 6);
        s.len = {70000, 66000, 1}, s.ws = {ends_of({100, 30000, 70000}), WriteSpec(), ends_of({1})};
        v.push_back(s);
    }
    for (int level : {1, 6})
        for (bool at_read : {true, false}) {
            // a run of an incremental stream that goes on in the bulk pipeline: 40 000 bytes of history, then 200 000 new ones
            Shape s = one("", 240000, level);
            s.name = std::string("resumed run at level ") + (level == 1 ? "1" : "6") + (at_read ? ", at a read" : ", in the middle of a Write");
            s.incremental = true, s.ro.resume = true, s.ro.at_read = at_read, s.ro.final_run = false;
            s.ro.p0 = 40000, s.ro.E0 = at_read ? 40000 : 50000, s.ro.base0 = 0, s.ro.abs_off = 123456, s.ro.start_block = 39000, s.ro.slot = 3, s.ro.start_syms = 17;
            s.ws = {ends_of({240000})};
            if (level == 1 && !at_read) s.want_err = "the run cannot go on in the bulk pipeline from where the literal engine stopped";
            v.push_back(s);
        }
    {
        Shape s = one("first run", 300000, 1);  // the first run of a stream that flushes: one Write, the flush at its end
        s.incremental = true, s.ro.final_run = false, s.ws = {writes_of(300000, 300000, 2)};
        v.push_back(s);
        s = one("continued run", 70000, 6);
        s.incremental = true, s.ro.cont = true, s.ro.hist = 65536, s.ro.abs_off = 1 << 20, s.ws = {ends_of({(1 << 20) + 70000})};
        v.push_back(s);
    }
    return v;
}

// A shape planned: the arguments (with arrays of their own), the plan, its layout.
struct Planned {
    std::vector<const void *> in;
    std::vector<void *> out;
    std::vector<int64_t> cap;
    std::vector<const WriteSpec *> wp;
    FoldedWrites folded;
    PlanArgs a;
    Plan pl;
    PlanLayout lay;
    bool ok = false;
    std::string err;
};
std::unique_ptr<Planned> plan_shape(const Shape &s, const PlanEnv &env, uintptr_t base = 0x100000000ull) {
    std::unique_ptr<Planned> p(new Planned());
    const int n = (int)s.len.size();
    for (int i = 0; i < n; i++) {
        p->in.push_back((const void *)(base + (uintptr_t)i * 0x1000000u));
        p->out.push_back((void *)(base + 0x80000000u + (uintptr_t)i * 0x1000000u));
        p->cap.push_back(s.len[(size_t)i] + s.len[(size_t)i] / 8 + 1024);
    }
    bool any_writes = false;
    for (size_t i = 0; i < s.ws.size(); i++) p->wp.push_back(s.ws[i].ends.empty() ? nullptr : &s.ws[i]), any_writes = any_writes || !s.ws[i].ends.empty();
    PlanArgs &a = p->a;
    a.n = n, a.in = p->in.data(), a.in_len = s.len.data(), a.out = p->out.data(), a.out_cap = p->cap.data(), a.level = s.level, a.strategy = s.strategy;
    a.force_seq = s.force_seq, a.ro = s.incremental ? &s.ro : nullptr;
    a.writes = fold_rle_writes(p->folded, n, s.len.data(), s.ws.empty() ? nullptr : p->wp.data(), any_writes, s.level, s.strategy, s.incremental, env);
    p->ok = plan_streams(p->pl, a, env, p->err);
    if (p->ok) plan_layout(p->lay, p->pl, a);
    return p;
}
const Shape &shape(const std::vector<Shape> &v, const char *name) {
    for (const Shape &s : v)
        if (s.name == name) return s;
    printf("FAIL: no shape %s\n", name);
    exit(1);
}

template <class T>
bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}
// everything of two plans but the caller's pointers in the descriptors
bool same_plan(const Plan &a, const Plan &b) {
    std::vector<StreamDesc> sa = a.sd, sb = b.sd;
    for (StreamDesc &s : sa) s.in = nullptr, s.out = nullptr;
    for (StreamDesc &s : sb) s.in = nullptr, s.out = nullptr;
    bool ok = same(sa, sb);
    for (int l = 0; l < kWorkLists; l++) ok = ok && a.list(l)->pre == b.list(l)->pre;
    return ok && a.n_pos == b.n_pos && a.n_syms == b.n_syms && a.n_chunks == b.n_chunks && a.n_segs == b.n_segs && a.n_sups == b.n_sups && a.n_blocks == b.n_blocks &&
           a.n_pieces == b.n_pieces && a.n_runs == b.n_runs && a.n_spec == b.n_spec && a.max_spec_n == b.max_spec_n && a.n_spec_streams == b.n_spec_streams &&
           a.any_fv == b.any_fv && a.any_rle == b.any_rle && a.any_dual == b.any_dual && a.n_rle_tiles == b.n_rle_tiles && a.lit_bytes == b.lit_bytes &&
           a.link_span == b.link_span && same(a.fr_chunks, b.fr_chunks) && a.fr_prov == b.fr_prov && a.fr_max_n == b.fr_max_n && a.n_cuts == b.n_cuts &&
           a.seg_c0 == b.seg_c0 && a.seg_after == b.seg_after && a.seg_base == b.seg_base && a.seg_S == b.seg_S && a.seg_cl == b.seg_cl && a.cstart == b.cstart &&
           a.head == b.head && a.cl == b.cl && same(a.plan_blk, b.plan_blk) && a.plan_wr_blk == b.plan_wr_blk;
}
bool same_layout(const PlanLayout &a, const PlanLayout &b) {
    return a.sd_bytes == b.sd_bytes && a.pre_bytes == b.pre_bytes && a.geo_bytes == b.geo_bytes && a.up_bytes == b.up_bytes && a.o_segcl == b.o_segcl &&
           a.o_cstart == b.o_cstart && a.o_head == b.o_head && a.o_cl == b.o_cl && memcmp(a.work, b.work, sizeof a.work) == 0 && a.wr_n == b.wr_n &&
           a.wr_off == b.wr_off && a.wr_bytes == b.wr_bytes;
}

// the offsets, the work lists, the table sizes, and the staged and bound plan of one shape
void check_invariants(const Shape &sh, Planned &p) {
    const std::string at = sh.name + ": ";
    Plan &pl = p.pl;
    const PlanLayout &lay = p.lay;
    const int n = p.a.n;
    int64_t pos = 0, sym = 0, chunk = 0, seg = 0, sup = 0, blk = 0, adler = 0, run = 0, cut = 0, spec = 0;
    int64_t want[kWorkLists] = {};
    bool offs = true, aligned = true, lists = true;
    for (int i = 0; i < n; i++) {
        const StreamDesc &s = pl.sd[(size_t)i];
        const int64_t len = sh.len[(size_t)i];
        offs = offs && s.pos_off == pos && s.sym_off == sym && s.chunk_off == chunk && s.seg_off == seg && s.sup_off == sup && s.blk_off == blk && s.adler_off == adler &&
               s.run_off == run && s.cut_off == cut && (s.spec_off == spec || pl.n_spec == 0) && s.n == len;
        aligned = aligned && s.pos_off % 64 == 0;
        pos += (len + 64 + 63) & ~63LL, sym += len + 64 + (sh.incremental ? kLitBufsize : 0), chunk += s.nchunks, seg += s.nsegs, sup += (s.nsegs + kSupSegs - 1) / kSupSegs;
        blk += s.max_blocks, adler += s.n_adler, run += s.run_slots, cut += s.cut_cap, spec += s.spec_n;
        const int64_t per[kWorkLists] = {(s.out_cap + 65535) / 65536,
                                         s.n_adler,
                                         (s.body_end >= 0 || s.fast_runs > 0 || s.fv_end >= 0) && len > 5 ? (len - 5 + pl.link_span - 1) / pl.link_span : 0,
                                         s.body_end >= 0 ? s.body_end / kMatchTile + 1 : 0,
                                         s.body_end >= 0 ? s.nchunks : 0,
                                         s.body_end >= 0 ? s.nsegs : 0,
                                         s.body_end >= 0 && s.nsegs > kSupSegs ? (s.nsegs + kSupSegs - 1) / kSupSegs : 0,
                                         s.max_blocks,
                                         s.fast_runs};
        for (int l = 0; l < kWorkLists; l++) {
            const std::vector<int32_t> &pre = pl.list(l)->pre;
            lists = lists && (int)pre.size() == n + 1 && pre[(size_t)i] == want[l] && pre[(size_t)i + 1] - pre[(size_t)i] == per[l];
            want[l] += per[l];
        }
    }
    expect(offs, at + "every stream's offsets are the sums of the earlier streams' counts");
    expect(aligned, at + "pos_off is a multiple of 64");
    expect(pos == pl.n_pos && sym == pl.n_syms && chunk == pl.n_chunks && seg == pl.n_segs && sup == pl.n_sups && blk == pl.n_blocks && adler == pl.n_pieces &&
               run == pl.n_runs && cut == pl.n_cuts && spec == pl.n_spec,
           at + "the plan's totals are the sums of the streams' counts");
    expect(lists, at + "every work list holds each stream's count, and n + 1 prefixes");
    size_t items = 0;
    bool work_ok = true;
    for (int l = 0; l < kWorkLists; l++) work_ok = work_ok && lay.work[l] == items && pl.list(l)->size() == (size_t)want[l], items += pl.list(l)->size();
    expect(work_ok && lay.work[kWorkLists] == items, at + "the work array holds the lists back to back");
    const size_t ns = (size_t)pl.n_segs, nc = (size_t)pl.n_chunks;
    expect(pl.seg_c0.size() == ns && pl.seg_after.size() == ns && pl.seg_base.size() == ns && pl.seg_S.size() == ns && pl.seg_cl.size() == ns + (size_t)n &&
               pl.cstart.size() == nc + (size_t)n && pl.head.size() == nc,
           at + "the tables have the sizes the layout counts on");
    expect(lay.sd_bytes == sizeof(StreamDesc) * (size_t)n && lay.pre_bytes == 4 * (size_t)kWorkLists * (size_t)(n + 1) && lay.o_segcl == 16 * ns &&
               lay.o_cstart == lay.o_segcl + 4 * (ns + (size_t)n) && lay.o_head == lay.o_cstart + 4 * (nc + (size_t)n) && lay.o_cl == lay.o_head + 4 * nc &&
               lay.geo_bytes == lay.o_cl + 4 * pl.cl.size() && lay.up_bytes == lay.sd_bytes + lay.pre_bytes + lay.geo_bytes,
           at + "the layout is the tables back to back behind descriptors and prefixes");
    // unbound: the pointers the planner cannot know are null, plan_blk an offset
    bool unbound = true;
    for (const StreamDesc &s : pl.sd)
        unbound = unbound && !s.seg_c0 && !s.seg_after && !s.seg_base && !s.seg_S && !s.seg_cl && !s.cl && !s.cstart && !s.head && !s.ins_bits && !s.wr_end && !s.wr_blk &&
                  !s.wr_flush && (uintptr_t)s.plan_blk <= pl.plan_blk.size();
    expect(unbound, at + "the planner leaves the device pointers null and plan_blk an offset");
    // bound to plain memory and staged there: every descriptor points at its own stream's part of what was staged
    std::vector<uint8_t> up(lay.up_bytes + 64, 0xEE), wr(lay.wr_bytes + 64, 0);
    std::vector<uint32_t> bits((size_t)pl.n_pos / 32 + 1);
    std::vector<BlockRec> blocks = pl.plan_blk;
    const bool has_wr = p.a.any_writes();
    plan_bind(pl, lay, p.a, up.data(), pl.any_fv ? bits.data() : nullptr, blocks.empty() ? nullptr : blocks.data(), has_wr ? wr.data() : nullptr);
    plan_stage(up.data(), pl, lay, n);
    if (has_wr) plan_stage_writes(wr.data(), pl, lay, p.a);
    expect(memcmp(up.data(), pl.sd.data(), lay.sd_bytes) == 0, at + "the staged descriptors are the bound ones");
    bool pre_ok = true, tabs = true, wr_ok = true, blk_ok = true;
    for (int l = 0; l < kWorkLists; l++) pre_ok = pre_ok && memcmp(up.data() + lay.sd_bytes + 4 * (size_t)l * (size_t)(n + 1), pl.list(l)->pre.data(), 4 * (size_t)(n + 1)) == 0;
    expect(pre_ok, at + "the staged prefixes are the work lists'");
    size_t first_blk = 0;
    for (int i = 0; i < n; i++) {
        const StreamDesc &s = pl.sd[(size_t)i];
        for (int k = 0; k < s.nsegs; k++) {
            const size_t g = (size_t)(s.seg_off + k);
            tabs = tabs && s.seg_c0[k] == pl.seg_c0[g] && s.seg_after[k] == pl.seg_after[g] && s.seg_base[k] == pl.seg_base[g] && s.seg_S[k] == pl.seg_S[g];
        }
        for (int k = 0; k <= s.nsegs; k++) tabs = tabs && s.seg_cl[k] == pl.seg_cl[(size_t)(s.seg_off + i + k)] && (size_t)s.seg_cl[k] <= pl.cl.size();
        for (int k = s.seg_cl[0]; k < s.seg_cl[s.nsegs]; k++) tabs = tabs && s.cl[k] == pl.cl[(size_t)k];
        for (int k = 0; k <= s.nchunks; k++) tabs = tabs && s.cstart[k] == pl.cstart[(size_t)(s.chunk_off + i + k)];
        for (int k = 0; k < s.nchunks; k++) tabs = tabs && s.head[k] == pl.head[(size_t)(s.chunk_off + k)];
        if (s.body_end >= 0) tabs = tabs && s.cstart[0] == s.start_pos && s.cstart[s.nchunks] == s.body_end + 1;
        if (s.fv_end >= 0) tabs = tabs && s.ins_bits == bits.data() + s.pos_off / 32;
        if (s.plan_nblk) blk_ok = blk_ok && s.plan_blk == blocks.data() + first_blk && s.plan_blk[s.plan_nblk - 1].eof == 1;
        first_blk += (size_t)s.plan_nblk;
        const WriteSpec *w = p.a.writes ? p.a.writes[i] : nullptr;
        if (write_block_wanted(w, sh.incremental)) {
            wr_ok = wr_ok && s.n_wr == (int32_t)w->ends.size() && (const uint8_t *)s.wr_end == wr.data() + lay.wr_off[(size_t)i];
            for (size_t k = 0; k < w->ends.size(); k++) wr_ok = wr_ok && s.wr_end[k] == w->ends[k] && (!s.wr_flush || s.wr_flush[k] == w->flush[k]);
            wr_ok = wr_ok && ((w->flushing() || sh.incremental) == (s.wr_flush != nullptr)) && ((s.wr_flush != nullptr) == (s.wr_blk != nullptr));
        } else
            wr_ok = wr_ok && !s.wr_end && !s.wr_flush && !s.wr_blk;
    }
    expect(tabs, at + "bound and staged, seg_c0 .. cl, cstart and head of every stream are its own entries");
    expect(blk_ok, at + "a stored stream's block list is its part of the batch's, the last block the final one");
    expect(wr_ok, at + "a stream's Write table block holds its ends and flush modes");
}
}  // namespace

int main() {
    const std::vector<Shape> shapes = edge_shapes();
    const PlanEnv def;
    // ---- equal keys, equal plans: the same arguments at other addresses; and the invariants of every shape ----
    for (const Shape &sh : shapes) {
        std::unique_ptr<Planned> a = plan_shape(sh, def), b = plan_shape(sh, def, 0x7000000000ull);
        if (!sh.want_err.empty()) {
            expect(!a->ok && a->err == sh.want_err && !b->ok, sh.name + ": refused, with the planner's one message");
            continue;
        }
        expect(a->ok && b->ok && a->err.empty(), sh.name + ": plans");
        if (!a->ok || !b->ok) continue;
        if (!sh.incremental) {
            PlanKey ka, kb;
            plan_key_fill(ka, a->a.n, sh.len.data(), a->cap.data(), sh.level, sh.strategy, 0, 0, false, false, false, false, sh.ws.empty() ? nullptr : a->wp.data(), def);
            plan_key_fill(kb, b->a.n, sh.len.data(), b->cap.data(), sh.level, sh.strategy, 0, 0, false, false, false, false, sh.ws.empty() ? nullptr : b->wp.data(), def);
            expect(plan_key_equal(ka, kb), sh.name + ": the two calls have equal keys");
        }
        expect(same_plan(a->pl, b->pl) && same_layout(a->lay, b->lay), sh.name + ": equal arguments at other addresses give the same plan and layout");
        expect(a->pl.sd[0].in == a->in[0] && b->pl.sd[0].in == b->in[0] && a->pl.sd[0].out == a->out[0] && a->pl.sd[0].in != b->pl.sd[0].in,
               sh.name + ": each plan has its own call's pointers");
        check_invariants(sh, *a);
    }
    // ---- the paths the edge shapes are there for ----
    auto P = [&](const char *name, const PlanEnv &e = PlanEnv()) { return plan_shape(shape(shapes, name), e); };
    expect(P("walk")->pl.n_spec == 1024 && P("1 MiB - 1 at level 6 (below the walk)")->pl.n_spec == 0, "the walk begins at 1 MiB");
    expect(P("length 523 at level 6")->pl.sd[0].body_end < 0 && P("length 524 at level 6")->pl.sd[0].body_end == 262, "the bulk parse begins at 524 bytes");
    expect(P("length 261 at level 1")->pl.sd[0].fv_end < 0 && P("length 262 at level 1")->pl.sd[0].fv_end == 0, "the sweeps begin at 262 bytes");
    expect(P("length 261 at level 6")->pl.lit_bytes == 0 && P("length 1 at level 6")->pl.lit_bytes == 0, "a stream below 262 bytes is the tail engine's alone");
    expect(P("length 65536 at level 6")->pl.sd[0].kl == 0 && P("length 65537 at level 6")->pl.sd[0].kl == 1, "the first refill comes with byte 65 537");
    expect(P("dual")->pl.any_dual && P("dual")->pl.any_fv && P("dual")->pl.n_runs > 0, "4 x 300 000 at level 1 are planned for the sweeps and the runs");
    expect(!P("dual struck")->pl.any_dual && P("dual struck")->pl.n_runs == 0 && P("dual struck")->pl.sd[0].fv_end >= 0, "a stream of 100 bytes among them: planned again, for the sweeps");
    {
        // (by default a stream of 100 bytes bars the double plan from the start; with ZS_FAST_MIN_INPUT=0 the batch is planned for
        // both first, the short stream takes neither, and the second pass plans what the default environment plans)
        PlanEnv low;
        low.has_fast_min_input = true, low.fast_min_input = 0;
        expect(P("dual", low)->pl.any_dual && !P("dual struck", low)->pl.any_dual && same_plan(P("dual struck", low)->pl, P("dual struck")->pl),
               "the double plan, struck by a stream it does not take, is the plan of the pass without it");
    }
    expect(P("one long stream among 5000 short ones")->pl.n_spec == 0 && P("one long stream among 5000 short ones")->pl.sd[2500].spec == 0, "the speculative grid is refused");
    expect(P("rle")->pl.any_rle && P("rle writes")->pl.any_rle && P("rle writes")->pl.sd[0].n_wr == 1, "Rle: Write ends away from the window ends fold into one Write");
    expect(!P("rle, a Write end 100 bytes below a window end")->pl.any_rle && P("rle, a Write end 300 bytes below a window end")->pl.any_rle, "Rle: a Write end within 262 bytes below a window end keeps its list");
    expect(P("level 0")->pl.plan_blk.size() >= 2 && P("level 0, flushing Writes")->pl.plan_wr_blk.size() == 4 && P("level 0, Writes without a flush")->pl.plan_wr_blk.empty(), "level 0: the stored blocks, and the blocks before each flushed Write");
    expect(P("copyto")->pl.sd[0].fv_end >= 0 && P("level 1, Writes of 5 bytes")->pl.sd[0].fv_end < 0 && P("level 1, Writes of 5 bytes")->pl.lit_bytes > 0, "level 1: 81 920-byte Writes take the sweeps, 5-byte Writes the literal engine");
    expect(P("64 streams")->pl.w_blocks.size() == 64 * 4 && P("65 streams")->pl.sd[64].n == 0, "64 and 65 streams");
    for (const char *name : {"resumed run at level 6, at a read", "resumed run at level 6, in the middle of a Write", "resumed run at level 1, at a read"}) {
        std::unique_ptr<Planned> p = P(name);
        expect(p->ok && p->pl.sd[0].resume == 1 && p->pl.sd[0].start_pos == 40000 && p->pl.sd[0].persist_off == 123456 && p->pl.sd[0].n_adler == 0, std::string(name) + ": goes on in the bulk pipeline");
        expect(p->ok && p->pl.sd[0].mid_write == (shape(shapes, name).ro.at_read ? 0 : 1), std::string(name) + ": mid_write is set unless the run begins at a read");
    }
    // ---- every switch of the planner is live: a shape whose plan differs from the default environment's, and the field that does ----
    struct Live {
        const char *sw, *shape_name, *field;
        std::function<void(PlanEnv &)> set;
        std::function<bool(const Plan &, const Plan &)> differs;  // (default, switched)
    };
    const std::vector<Live> live = {
        {"no_rle_multi", "rle writes", "sd[0].rle_end", [](PlanEnv &e) { e.no_rle_multi = true; }, [](const Plan &d, const Plan &s) { return d.sd[0].rle_end >= 0 && s.sd[0].rle_end < 0; }},
        {"no_rle_runs", "rle", "sd[0].rle_end", [](PlanEnv &e) { e.no_rle_runs = true; }, [](const Plan &d, const Plan &s) { return d.sd[0].rle_end >= 0 && s.sd[0].rle_end < 0; }},
        {"no_fast_vec", "sweeps", "sd[0].fv_end", [](PlanEnv &e) { e.no_fast_vec = true; }, [](const Plan &d, const Plan &s) { return d.sd[0].fv_end >= 0 && s.sd[0].fv_end < 0; }},
        {"fast_no_rounds", "sweeps", "fr_chunks", [](PlanEnv &e) { e.fast_no_rounds = true; }, [](const Plan &d, const Plan &s) { return !d.fr_chunks.empty() && s.fr_chunks.empty() && s.any_fv; }},
        {"no_spec", "walk", "n_spec", [](PlanEnv &e) { e.no_spec = true; }, [](const Plan &d, const Plan &s) { return d.n_spec > 0 && s.n_spec == 0; }},
        {"no_fast_multi", "copyto", "sd[0].fv_end", [](PlanEnv &e) { e.no_fast_multi = true; }, [](const Plan &d, const Plan &s) { return d.sd[0].fv_end >= 0 && s.sd[0].fv_end < 0; }},
        {"no_fast_resume", "first run", "sd[0].fv_end", [](PlanEnv &e) { e.no_fast_resume = true; }, [](const Plan &d, const Plan &s) { return d.sd[0].fv_end >= 0 && s.sd[0].fv_end < 0; }},
        {"no_resume_rounds", "resumed run at level 1, at a read", "fr_chunks", [](PlanEnv &e) { e.no_resume_rounds = true; }, [](const Plan &d, const Plan &s) { return !d.fr_chunks.empty() && s.fr_chunks.empty() && s.any_fv; }},
        {"has_fr_ratio / fr_ratio = 0", "sweeps", "fr_chunks", [](PlanEnv &e) { e.has_fr_ratio = true, e.fr_ratio = 0; }, [](const Plan &d, const Plan &s) { return !d.fr_chunks.empty() && s.fr_chunks.empty(); }},
        {"has_fr_chunk / fr_chunk = 4096", "sweeps", "fr_chunks.size()", [](PlanEnv &e) { e.has_fr_chunk = true, e.fr_chunk = 4096; }, [](const Plan &d, const Plan &s) { return !s.fr_chunks.empty() && s.fr_chunks.size() < d.fr_chunks.size(); }},
        {"has_fast_chunk / fast_chunk = 262144", "sweeps", "sd[0].fast_runs", [](PlanEnv &e) { e.has_fast_chunk = true, e.fast_chunk = 262144; }, [](const Plan &d, const Plan &s) { return d.sd[0].fast_runs == 5 && s.sd[0].fast_runs == 2; }},
        {"has_spec_len / spec_len = 512", "walk", "sd[0].spec_n", [](PlanEnv &e) { e.has_spec_len = true, e.spec_len = 512; }, [](const Plan &d, const Plan &s) { return d.sd[0].spec_n == 1024 && s.sd[0].spec_n == 2048; }},
        {"has_spec_min / spec_min = 2097152", "walk", "n_spec", [](PlanEnv &e) { e.has_spec_min = true, e.spec_min = 2097152; }, [](const Plan &d, const Plan &s) { return d.n_spec > 0 && s.n_spec == 0; }},
        {"has_fast_min_input / fast_min_input = 4194304", "sweeps", "any_dual", [](PlanEnv &e) { e.has_fast_min_input = true, e.fast_min_input = 4194304; }, [](const Plan &d, const Plan &s) { return d.any_dual && !s.any_dual && s.n_runs == 0; }},
    };
    for (const Live &l : live) {
        PlanEnv e;
        l.set(e);
        std::unique_ptr<Planned> d = P(l.shape_name), s = P(l.shape_name, e);
        expect(d->ok && s->ok && l.differs(d->pl, s->pl) && !same_plan(d->pl, s->pl), std::string(l.sw) + " changes " + l.field + " of the plan of \"" + l.shape_name + "\"");
    }
    {
        // in the key, not the planner's (zs_plan_key.h says why): no plan depends on them
        PlanEnv e;
        e.no_live_list = true, e.has_spec_warm = true, e.spec_warm = 0;
        bool unread = true;
        for (const Shape &sh : shapes)
            if (sh.want_err.empty()) unread = unread && same_plan(plan_shape(sh, def)->pl, plan_shape(sh, e)->pl);
        expect(unread, "no_live_list and spec_warm change no plan");
    }
    // ---- the values the engine makes of the switches, at the edges of their strings' values ----
    {
        PlanEnv e;
        expect(plan_spec_bits(e) == kSpecLenBits && plan_spec_warm(e) == kSpecWarm && plan_spec_min(e) == kSpecMinInput && plan_fast_min_input(e) == kFastMinPeriodic, "nothing set: the defaults");
        e.has_spec_len = e.has_spec_warm = e.has_spec_min = true, e.spec_len = -1, e.spec_warm = -1, e.spec_min = -1;
        expect(plan_spec_bits(e) == kSpecLenBits && plan_spec_warm(e) == 0 && plan_spec_min(e) == kWindowSize, "-1: the default length, no warm-up, 64 KiB");
        e.spec_len = 2048, e.spec_warm = 100000, e.spec_min = 0;
        expect(plan_spec_bits(e) == 11 && plan_spec_warm(e) == 4096 && plan_spec_min(e) == kWindowSize, "2048 / a warm-up beyond 4096 / a minimum of 0");
        e.has_fast_chunk = true, e.fast_chunk = 0;
        expect(plan_run_chunk(e, 1 << 30) == 65536, "ZS_FAST_CHUNK=0: 64 KiB");
        e.fast_chunk = 1 << 30;
        expect(plan_run_chunk(e, 0) == kFastChunk && plan_run_chunk(PlanEnv(), 0) == 65536 && plan_run_chunk(PlanEnv(), 1ll << 30) == kFastChunk, "a run's share: 64 .. 256 KiB");
        e.has_fr_chunk = true, e.fr_chunk = -1;
        expect(plan_fr_target(e, 1 << 30) == 2048 && plan_fr_target(PlanEnv(), 1 << 30) == kFsChunkMax && plan_fr_target(PlanEnv(), 0) == 2048, "the rounds' chunks: 2048 .. 10 240 positions");
    }
    printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "PASS", checks, failures);
    return failures ? 1 : 0;
}
