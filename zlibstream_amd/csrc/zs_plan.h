// zs_plan.h -- the planner of a deflate call: which path every stream takes, the descriptors, the work lists and the parse
// tables (plan_streams), where they lie in the one buffer that is uploaded (plan_layout), the pointers into it (plan_bind) and
// the copy into the staging area (plan_stage).  No HIP call and no look at the environment in here: the switches come in the
// PlanEnv of the call's key (zs_plan_key.h), so a plan depends on nothing the key does not hold.  The engine (zs_engine.hip)
// allocates, uploads and launches; tests/cpp/test_plan.cpp runs all of this on the host.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "zs_device.h"
#include "zs_plan_key.h"

namespace zs {

// A kernel's work items: (stream, index) for index < count(stream), stream after stream.  The host keeps the running totals
// (one per stream); the pairs themselves are written on the device (zs_worklist_kernel) -- for a 64 MiB stream they are
// 46 K pairs, whose making and upload were 0.1 ms of host time per call.
// (begin, a count per stream, finish: a store per stream.  Grown entry by entry the nine lists were nine calls a stream that
// the planner as a function of its own no longer had inlined: 5 % of a planning call of 4096 streams.)
struct WorkList {
    std::vector<int32_t> pre;  // pre[i] = items of the streams before i; one more entry = the total
    void begin(int n) { pre.assign((size_t)n + 1, 0); }
    // once per stream at the most; pre holds the streams' own counts, and size() / empty() mean nothing, until finish()
    void add(int stream, int64_t count) { pre[(size_t)stream + 1] = (int32_t)count; }
    void finish() {
        for (size_t i = 1; i < pre.size(); i++) pre[i] += pre[i - 1];
    }
    size_t size() const { return pre.empty() ? 0 : (size_t)pre.back(); }
    bool empty() const { return size() == 0; }
};
constexpr int kWorkLists = 9;
struct Plan {
    std::vector<StreamDesc> sd;
    WorkList w_clear, w_adler, w_links, w_match, w_chunks, w_segs, w_sups, w_blocks, w_runs;
    WorkList *list(int l) {
        WorkList *const lists[kWorkLists] = {&w_clear, &w_adler, &w_links, &w_match, &w_chunks, &w_segs, &w_sups, &w_blocks, &w_runs};
        return lists[l];
    }
    const WorkList *list(int l) const { return const_cast<Plan *>(this)->list(l); }
    int64_t n_pos = 0, n_syms = 0;
    int64_t n_chunks = 0, n_segs = 0, n_sups = 0, n_blocks = 0, n_pieces = 0, n_runs = 0;
    int64_t n_spec = 0;  // chunks of the speculative grid, all streams that try the speculative walk
    int max_spec_n = 0, n_spec_streams = 0;
    bool any_fv = false, any_rle = false;
    bool any_dual = false;  // levels 1-3, a few streams below 4 MiB: planned for the sweeps and for the speculative runs, the links decide (zs_fast_probe_kernel)
    int64_t n_rle_tiles = 0;
    int64_t lit_bytes = 0;           // input bytes of this plan that only the literal engine parses
    int64_t link_span = 0;           // positions per workgroup of the link kernel
    std::vector<FsChunk> fr_chunks;  // levels 1-3 as rounds over the chunks of the streams (zs_fast_sweep.h "Rounds"); empty: one workgroup per stream
    size_t fr_prov = 0;              // symbols of room in the chunks' provisional buffer
    int fr_max_n = 0;                // the most chunks a stream has
    int64_t n_cuts = 0;     // entries of a cut list (batched cut rounds): one per read boundary
    // parse-segment tables (zs_core.h build_geometry), all streams: per segment (seg_off order); seg_cl and cstart hold one
    // entry more per stream (stream i's lists begin at seg_off + i / chunk_off + i); seg_cl's values index `cl`
    std::vector<int32_t> seg_c0, seg_after, seg_base, seg_S, seg_cl, cstart, head;
    std::vector<uint32_t> cl;
    std::vector<BlockRec> plan_blk;                    // level 0: the stored blocks of every stream, stream after stream
    std::vector<int32_t> plan_wr_blk;                  // level 0 under a flush mode: blocks flushed before each Write began
};

// What the planning reads of one run of an incremental stream (zs_engine.hip RunOpts, which adds what a run gives back).
// final_run == false: the stream goes on after this run's Writes, the engine is left in `persist` (device memory) where
// Deflate.Compress would return to its caller, and only what is final -- whole blocks and flush markers, complete bytes -- is
// output.  cont: the run continues from `persist`; the input buffer then holds the stream from position abs_off on (64 KiB
// already read, then the new bytes) and `writes` holds absolute ends.
struct PlanRun {
    bool final_run = true, cont = false;
    int64_t hist = 0;  // leading bytes of the buffer that earlier runs have parsed (history: up to 64 KiB)
    LitPersist *persist = nullptr;
    int64_t abs_off = 0;
    uint32_t adler_stream = 1, carry_byte = 0;
    // cont: the literal engine stops at the first clean loop-top at or behind this stream position (< 0: runs on) ...
    int64_t stop_abs = -1;
    // ... and the run behind such a stop goes on from there on the bulk pipeline (`resume`): loop-top p0 with the input read up to
    // E0, the window at base0, the block in progress begun at start_block -- buffer positions, the buffer beginning at
    // stream position abs_off -- with start_syms symbols, in the lazy parse's node `slot` of a chunk that begins at p0
    // at_read: the stream was flushed at p0 (E0 == p0, nothing pending): the run's first pass through the loop reads, like a
    // stream's first one, and the run begins with a new Deflate call
    bool resume = false, mid_write = false, at_read = false;
    int64_t p0 = 0, E0 = 0, base0 = 0, start_block = 0;
    int slot = 0;
    uint32_t start_syms = 0;
};

// The arguments of a call as the planner takes them.  `writes` (optional): one entry per stream, the Writes of a multi-Write
// stream (null: the stream is one Write), Rle lists folded already (fold_rle_writes).  no_rounds: the call is barred from the
// sweeps' rounds (the call before gave them up).
struct PlanArgs {
    int n = 0;
    const void *const *in = nullptr;
    const int64_t *in_len = nullptr;
    void *const *out = nullptr;
    const int64_t *out_cap = nullptr;
    int level = 6, strategy = 0;  // (level -1 is 6 by now)
    const WriteSpec *const *writes = nullptr;
    int force_seq = 0;
    const PlanRun *ro = nullptr;
    bool rounds = false;
    const std::vector<uint8_t> *force_lit = nullptr;
    bool no_rounds = false;
    bool any_writes() const {
        for (int i = 0; i < n && writes; i++)
            if (writes[i]) return true;
        return false;
    }
};

// ---- what the engine makes of the switches: the planner and the launches call these, nobody parses a string twice ----
// The speculative chunk walk.  ZS_SPEC_LEN / ZS_SPEC_WARM / ZS_SPEC_MIN: the chunk length (512, 1024 or
// 2048), the warm-up and the shortest stream that tries it
inline int plan_spec_bits(const PlanEnv &e) {
    const int v = e.has_spec_len ? e.spec_len : 0;
    return v == 512 ? 9 : v == 2048 ? 11 : v == 1024 ? 10 : kSpecLenBits;
}
inline int plan_spec_warm(const PlanEnv &e) { return e.has_spec_warm ? std::max(0, std::min(4096, e.spec_warm)) : kSpecWarm; }
inline int64_t plan_spec_min(const PlanEnv &e) { return e.has_spec_min ? std::max<int64_t>(kWindowSize, e.spec_min) : kSpecMinInput; }
// a speculative run's share of its stream (levels 1-3, image-like data): a run is one wave on one CU, so a batch shorter than
// 256 runs of 256 KiB is cut finer, down to 64 KiB a run (64 KiB of warm-up in front of each: at most twice the work)
inline int plan_run_chunk(const PlanEnv &e, int64_t total_len) {
    return e.has_fast_chunk ? std::max(65536, std::min((int)kFastChunk, e.fast_chunk & ~65535))
                            : (int)std::max<int64_t>(65536, std::min<int64_t>(kFastChunk, ((total_len / 256 + 65535) >> 16) << 16));
}
// the rounds' chunks: 2048 positions or more (a run's fixed cost -- staging 32 K positions of history -- is 15-30 us, a sweep makes
// ~390 positions final in 8 us), at most what one staging of the tile covers; between the two, as many chunks as fit
// the chip at once: a round of 260 chunks takes the 256 CUs twice as long as one of 250
inline int64_t plan_fr_target(const PlanEnv &e, int64_t pos_fv) {
    const int64_t target = e.has_fr_chunk ? e.fr_chunk : pos_fv / 250;
    return target < 2048 ? 2048 : target > kFsChunkMax ? kFsChunkMax : target;
}
inline int64_t plan_fast_min_input(const PlanEnv &e) { return e.has_fast_min_input ? e.fast_min_input : kFastMinPeriodic; }

// CompressionStrategy.Rle does not look at Write ends: Deflate.Rle.cs leaves a Deflate call as soon as fewer than MAX_MATCH bytes
// are ahead under NoFlush (:24-38), so every match is measured with a full lookahead whatever the Writes are, and nothing is
// inserted anywhere.  What a Write end can move is the loop-top at which the window slides -- when it lies within 262 bytes
// below a window end -- and with it a block's permission to be stored.  Any other NoFlush schedule is the single Write's
// stream (checked against the oracle on random data and schedules, tests/test_oracle.py) and runs as one.
// Returns the call's Write lists with such streams' lists folded into one Write (`keep` owns what was made).
struct FoldedWrites {
    std::vector<WriteSpec> one;
    std::vector<const WriteSpec *> ptrs;
};
inline const WriteSpec *const *fold_rle_writes(FoldedWrites &keep, int n, const int64_t *in_len, const WriteSpec *const *writes, bool any_writes, int level, int strategy,
                                               bool incremental, const PlanEnv &env) {
    if (!(any_writes && strategy == kRle && level >= 1 && !incremental && !env.no_rle_multi)) return writes;
    keep.one.resize((size_t)n);
    keep.ptrs.assign(writes, writes + n);
    for (int i = 0; i < n; i++) {
        const WriteSpec *wr = writes[i];
        if (!wr || wr->ends.size() <= 1 || wr->flushing()) continue;
        bool safe = true;
        for (size_t k = 0; k + 1 < wr->ends.size() && safe; k++) {
            const int64_t E = wr->ends[k];
            safe = !(E >= kWindowSize - kMinLookahead && (E % kWSize) >= kWSize - kMinLookahead);
        }
        if (safe) {
            keep.one[(size_t)i] = *wr;
            keep.one[(size_t)i].ends.assign(1, in_len[i]);
            keep.one[(size_t)i].flush.assign(1, 0);
            keep.ptrs[(size_t)i] = &keep.one[(size_t)i];
        }
    }
    return keep.ptrs.data();
}

// One pass of the planner over the streams, with or without the double plan of levels 1-3 (plan_streams, below).
// Returns false with `err` set, or true with `dual_broken` saying that a stream did not take the double plan after all.
inline bool plan_pass(Plan &pl, const PlanArgs &a, const PlanEnv &env, const bool allow_dual, bool &dual_broken, std::string &err) {
    const int n = a.n, level = a.level, strategy = a.strategy, force_seq = a.force_seq;
    const int64_t *const in_len = a.in_len;
    const PlanRun *const ro = a.ro;
    const LevelCfg lv = level_cfg(level);
    const int64_t fast_min_input = plan_fast_min_input(env), spec_min = plan_spec_min(env);
    const int spec_bits = plan_spec_bits(env);
    pl = Plan();
    pl.sd.resize((size_t)n);
    for (int l = 0; l < kWorkLists; l++) pl.list(l)->begin(n);
    // positions per workgroup of the link kernel (each replays 32 Ki positions of warm-up first): long spans for a
    // big batch, shorter ones when that is what it takes to give every CU a workgroup
    int64_t total_len = 0;
    for (int i = 0; i < n; i++) total_len += in_len[i];
    const int64_t link_span = total_len >= (48ll << 20) ? 262144 : total_len >= (24ll << 20) ? 131072 : 65536;
    pl.link_span = link_span;
    const int run_chunk = plan_run_chunk(env, total_len);
    for (int i = 0; i < n; i++) {
        StreamDesc &s = pl.sd[(size_t)i];
        int64_t len = in_len[i];
        const WriteSpec *const wr = a.writes ? a.writes[i] : nullptr;  // this stream's own Writes
        s.in = (const uint8_t *)a.in[i];
        s.out = (uint8_t *)a.out[i];
        s.out_cap = a.out_cap[i];
        s.n = (int32_t)len;
        const bool multi = wr && wr->ends.size() > 1;
        // an incremental run always takes the block-by-block output accounting (its state is carried from run to run)
        const bool flushing = wr && (wr->flushing() || ro);
        const bool resume = ro && ro->resume;
        const bool cont = ro && ro->cont && !resume, final_run = !ro || ro->final_run;
        // the bulk pipeline takes the NoFlush schedules build_geometry accepts (zs_core.h: any Write sizes but streams written
        // a few bytes at a time); a stream the resolve kernel flagged (force_lit: a read whose pre-insert hashes bytes behind the
        // data) and other streams of several Writes run on the literal engine.  Levels 1-3 keep the single Write's events.
        std::vector<ReadEvent> rev;
        Geometry geo;
        const int64_t one_write[1] = {len};
        const bool lit_forced = a.force_lit && (*a.force_lit)[(size_t)i];
        const std::vector<int64_t> no_ends_;
        GeoStart gs;
        if (resume) gs.resume = true, gs.at_read = ro->at_read, gs.p0 = ro->p0, gs.E0 = ro->E0, gs.base0 = ro->base0;
        // (a flush mode on the run's last Write alone is the tail engine's business: it closes the block there)
        bool inner_flush = false;
        if (wr)
            for (size_t k = 0; k + 1 < wr->flush.size(); k++) inner_flush = inner_flush || wr->flush[k] != 0;
        const bool slow_ok = lv.func == 2 && strategy != kRle && !cont && !lit_forced && !(multi && inner_flush) &&
                             build_geometry(len, multi ? wr->ends : no_ends_, geo, gs);
        // levels 1-3 take several NoFlush Writes too when every read brings a full lookahead and no Write ends where its loop-top
        // may or may not slide the window (zs_core.h build_read_events: Stream.CopyTo's 81 920-byte Writes do; a Write every few
        // bytes does not)
        const bool fast_multi = multi && !inner_flush && !cont && !resume && lv.func == 1 && strategy != kRle && !env.no_fast_multi &&
                                build_read_events(len, wr->ends, rev, true);
        // levels 1-3 behind a flush (round 5): the run goes on from the suspended engine's chains too -- zs_import_chains_kernel's
        // links ARE DeflateFast's chains for the history (prev[] names inserted positions only), so with "inserted" for every
        // position the chains reach, the sweeps start at p0 as they start at 0; one Write, the engine standing at the flush
        // (several NoFlush Writes behind the flush as well, on the conditions of a stream's several Writes: every read brings a
        // full lookahead, no Write ends where its loop-top may or may not slide the window)
        const bool fast_resume = resume && ro->at_read && lv.func == 1 && strategy != kRle && !inner_flush && !lit_forced && !env.no_fast_resume &&
                                 len - ro->p0 >= 2 * kMinLookahead &&
                                 (multi ? build_read_events(len, wr->ends, rev, true, ro->p0, ro->base0)
                                        : build_read_events(len, std::vector<int64_t>(one_write, one_write + 1), rev, true, ro->p0, ro->base0));
        const bool regular = fast_resume ? true : cont ? false : multi ? fast_multi : build_read_events(len, std::vector<int64_t>(one_write, one_write + 1), rev);
        s.body_end = slow_ok ? (int32_t)geo.body_end : -1;
        // levels 1-3, one Write: the speculative chunk runs for large streams (they verify on periodic data and are parallel
        // inside a stream), else -- and when they did not verify (force_seq) -- DeflateFast for the lanes of a wave
        // (round 5: also the first run of a stream that flushes -- one Write, the flush at its end: the tail engine closes the
        // block and is left suspended as it is behind the slow levels' bulk runs)
        const bool fast_one = lv.func == 1 && strategy != kRle && regular && len >= kMinLookahead && !cont && !resume &&
                              ((!flushing && final_run && !ro && (!multi || fast_multi)) || (ro && (!multi || fast_multi) && !inner_flush && !lit_forced && !env.no_fast_resume));
        // (force_seq: 1 -- the runs did not verify, or the data does not look periodic: the sweeps; 2 -- they did not verify and the
        // stream is few symbols: one run of the engine for the whole stream, below)
        // (a run's buffers are 1.7 MB whatever the stream's length: streams below 4 MiB only in batches of a few -- allow_dual)
        // (HuffmanOnly: nothing is searched, every position a literal -- the sweeps take that at 7 GB/s, the runs' engine symbol by symbol)
        const bool fast_par = fast_one && !multi && force_seq != 1 && !ro && strategy != kHuffmanOnly &&
                              (len >= kFastMinInput || allow_dual || (force_seq == 2 && n <= 16 && len >= fast_min_input));
        if (allow_dual && !fast_par) dual_broken = true;
        s.fv_end = ((fast_one && (!fast_par || allow_dual) && !env.no_fast_vec) || fast_resume) ? (int32_t)(len - kMinLookahead) : -1;
        s.ins_bits = nullptr;
        if (s.fv_end >= 0) {
            pl.any_fv = true;
        }
        // CompressionStrategy.Rle, one Write: the parse is a function of where the runs of equal bytes begin (zs_rle.h)
        s.rle_end = -1, s.rle_tile_off = 0;
        s.fr_first = 0, s.fr_n = 0;
        if (strategy == kRle && level >= 1 && !multi && !flushing && final_run && !ro && regular && !env.no_rle_runs) {
            s.rle_end = (int32_t)rle_body_end(len);
            if (s.rle_end >= 0) {
                pl.any_rle = true;
                s.rle_tile_off = (int32_t)pl.n_rle_tiles;
                pl.n_rle_tiles += (s.rle_end + kMaxMatch + 1 + 4095) / 4096;
            }
        }
        s.n_wr = (multi || flushing) ? (int32_t)wr->ends.size() : 1;  // 0: a run without input (Finish alone)
        s.wr_end = nullptr;
        s.wr_flush = nullptr, s.wr_blk = nullptr, s.out_chunk = wr ? wr->chunk : 512, s.raw = wr && wr->raw;
        s.kl = num_refills(len - (resume ? ro->base0 : 0));
        s.resume = resume && (slow_ok || fast_resume) ? 1 : 0, s.cont_bits = (cont || resume) ? 1 : 0, s.mid_write = (ro && (ro->mid_write || (resume && !ro->at_read))) ? 1 : 0;
        if (resume && !slow_ok && !fast_resume) {
            err = "the run cannot go on in the bulk pipeline from where the literal engine stopped";
            return false;
        }
        s.start_slot = resume ? ro->slot : 0, s.start_syms = resume ? ro->start_syms : 0, s.base0 = resume ? ro->base0 : 0;
        s.start_block = resume ? ro->start_block : 0, s.start_pos = resume ? ro->p0 : 0, s.persist_off = resume ? ro->abs_off : 0, s.stop_abs = (ro && cont) ? ro->stop_abs : -1;
        s.nchunks = s.body_end >= 0 ? geo.nchunks() : 0;
        s.pos_off = pl.n_pos;
        pl.n_pos += (len + 64 + 63) & ~63LL;
        s.sym_off = pl.n_syms;
        pl.n_syms += len + 64 + (ro ? kLitBufsize : 0);  // a continued run starts with the symbols of the block in progress
        s.chunk_off = (int32_t)pl.n_chunks;
        pl.n_chunks += s.nchunks;
        s.seg_off = (int32_t)pl.n_segs;
        s.nsegs = 0;
        s.cut_off = (int32_t)pl.n_cuts, s.cut_cap = 0;
        s.grid_chunks = 0;
        if (s.body_end >= 0) {
            s.grid_chunks = 1;
            for (size_t k = 1; k + 1 < geo.cstart.size() && s.grid_chunks; k++)
                if (geo.cstart[k] != (int32_t)((int64_t)k * kChunk - (kMinLookahead - 1))) s.grid_chunks = 0;
            // ... and the segments those of a single Write's window ends (chunk_ctx's closed form for the chunk -> segment marks)
            if (geo.cstart.empty() || geo.cstart[0] != 0) s.grid_chunks = 0;
            for (size_t k = 0; k < geo.head.size() && s.grid_chunks; k++)
                if (geo.head[k] != ((k >= 32 && ((k - 32) & 15) == 0) ? (int32_t)((k - 32) >> 4) + 2 : 0)) s.grid_chunks = 0;
            s.cut_cap = (int32_t)(geo.cl.size() + (size_t)geo.nsegs() + 8);
            pl.n_cuts += s.cut_cap;
            s.nsegs = geo.nsegs();
            const int32_t cl0 = (int32_t)pl.cl.size();
            pl.seg_c0.insert(pl.seg_c0.end(), geo.seg_c0.begin(), geo.seg_c0.end());
            pl.seg_after.insert(pl.seg_after.end(), geo.seg_after.begin(), geo.seg_after.end());
            pl.seg_base.insert(pl.seg_base.end(), geo.seg_base.begin(), geo.seg_base.end());
            pl.seg_S.insert(pl.seg_S.end(), geo.seg_S.begin(), geo.seg_S.end());
            for (int32_t v : geo.seg_cl) pl.seg_cl.push_back(v + cl0);
            pl.cl.insert(pl.cl.end(), geo.cl.begin(), geo.cl.end());
            pl.cstart.insert(pl.cstart.end(), geo.cstart.begin(), geo.cstart.end());
            pl.head.insert(pl.head.end(), geo.head.begin(), geo.head.end());
        } else {
            if (fast_resume) {  // segment 0: the engine as the flush left it -- the data ends at p0, so the first event fires at the run's first loop-top
                // (an event's trigger is the data end before it - 261, and a negative one means "none": p0 below 261 counts as 261)
                pl.seg_c0.push_back(0), pl.seg_after.push_back((int32_t)std::max<int64_t>(ro->p0, kMinLookahead - 1)), pl.seg_base.push_back((int32_t)ro->base0);
                pl.seg_S.push_back(0), pl.seg_cl.push_back((int32_t)pl.cl.size());
                s.nsegs++;
            }
            if (s.fv_end >= 0 || s.rle_end >= 0)  // levels 1-3, Rle: the events of the single Write (the tail engine takes base and data end from them)
                for (size_t k = 0; k < rev.size(); k++) {
                    const int64_t at = (k || fast_resume) ? rev[k].at - (s.rle_end >= 0 ? kMaxMatch : kMinLookahead - 1) : 0;  // where the segment starts
                    if (at > (s.rle_end >= 0 ? s.rle_end : s.fv_end)) break;
                    pl.seg_c0.push_back(0), pl.seg_after.push_back((int32_t)rev[k].after), pl.seg_base.push_back((int32_t)rev[k].base);
                    pl.seg_S.push_back(0), pl.seg_cl.push_back((int32_t)pl.cl.size());
                    s.nsegs++;
                }
            pl.seg_cl.push_back((int32_t)pl.cl.size());
            pl.cstart.push_back(0);
        }
        // (the tables' device addresses: plan_bind)
        s.seg_c0 = s.seg_after = s.seg_base = s.seg_S = s.seg_cl = nullptr, s.cl = nullptr, s.cstart = nullptr, s.head = nullptr;
        pl.n_segs += s.nsegs;
        s.sup_off = (int32_t)pl.n_sups;
        pl.n_sups += (s.nsegs + kSupSegs - 1) / kSupSegs;
        // the speculative chunk walk in place of the maps: the slow levels' single Write from a minimum length on (a stream that
        // does not verify, or whose match tiles say it is periodic, goes to the maps as it always did)
        s.spec = 0, s.spec_n = 0, s.spec_off = (int32_t)pl.n_spec;
        bool spec_geo = s.body_end >= 0 && geo.body_end == len - kMinLookahead;
        if (spec_geo) {
            // the speculative grid's own closed form (spec_chunk_ctx): segment k >= 1 is the one window end 65536 + 32768 (k - 1),
            // whatever the 2048-position chunks of the map path look like
            const int64_t want = 1 + (len > kWindowSize ? (len - kWindowSize - 1) / kWSize + 1 : 0);
            spec_geo = (int64_t)geo.nsegs() == want && geo.seg_cl.size() == (size_t)want + 1 && geo.seg_cl[0] == 0 && geo.seg_cl[1] == 0;
            for (int64_t k = 1; k < want && spec_geo; k++)
                spec_geo = geo.seg_cl[(size_t)k + 1] - geo.seg_cl[(size_t)k] == 1 &&
                           geo.cl[(size_t)geo.seg_cl[(size_t)k]] == ((uint32_t)(kWindowSize + kWSize * (k - 1)) | kClWindowBit);
        }
        if (!env.no_spec && lv.func == 2 && (strategy == kDefault || strategy == kFiltered) && !wr && !ro && !lit_forced && spec_geo && len >= spec_min &&
            n <= 65535) {
            s.spec = 1, s.spec_n = (int32_t)((((int64_t)s.body_end + kMinLookahead - 1) >> spec_bits) + 1);
            pl.n_spec += s.spec_n, pl.n_spec_streams++;
            pl.max_spec_n = std::max(pl.max_spec_n, (int)s.spec_n);
        }
        // levels 1-3, one Write, large enough: speculative chunk runs instead of one sequential engine
        s.run_chunk = run_chunk;
        s.fast_runs = fast_par ? (force_seq == 2 ? 1 : (int32_t)((len + run_chunk - 1) / run_chunk)) : 0;
        s.run_slots = fast_par ? (force_seq == 2 ? (int32_t)((len + 4096) / kFastChunk + 1) : s.fast_runs) : 0;
        s.run_off = (int32_t)pl.n_runs;
        pl.n_runs += s.run_slots;
        pl.w_runs.add(i, s.fast_runs);
        s.blk_off = (int32_t)pl.n_blocks;
        // level 0 runs with memLevel 7: a block is flushed every 8191 symbols (only Rle tallies symbols there)
        s.max_blocks = (int32_t)(level == 0 ? len / 8191 + len / 32506 + 4 : len / kBlockSyms + 2);
        if (flushing) s.max_blocks += (int32_t)wr->ends.size() + 1;  // every Write under a flush mode closes a block
        s.plan_blk = nullptr, s.plan_nblk = 0;
        s.final_run = final_run ? 1 : 0, s.cont = cont ? 1 : 0, s.persist = ro ? ro->persist : nullptr;
        s.abs_off = (ro && !resume) ? ro->abs_off : 0, s.adler_stream = ro ? ro->adler_stream : 1, s.carry_byte = ro ? ro->carry_byte : 0;
        if (level == 0 && strategy != kRle && !ro) {
            // DeflateStored: block boundaries from the sizes alone (zs_core.h plan_stored_blocks); s.plan_blk holds the
            // offset into the batch's list until the device address is known
            const size_t first = pl.plan_blk.size();
            const std::vector<int64_t> no_ends;
            const std::vector<uint8_t> no_flush;
            if (flushing) pl.plan_wr_blk.assign(wr->ends.size(), 0);
            plan_stored_blocks(len, (multi || flushing) ? wr->ends : no_ends, flushing ? wr->flush : no_flush,
                               [&](int64_t start, int32_t blen, int can_store, int eof) {
                                   pl.plan_blk.push_back(BlockRec{start, 0, blen, 0, can_store, eof});
                               },
                               [&](int w, int nb) {
                                   if (flushing) pl.plan_wr_blk[(size_t)w] = nb;
                               });
            s.plan_nblk = (int32_t)(pl.plan_blk.size() - first);
            s.plan_blk = (const BlockRec *)(uintptr_t)first;
            s.max_blocks = s.plan_nblk + 1;
        }
        pl.n_blocks += s.max_blocks;
        s.adler_off = (int32_t)pl.n_pieces;
        s.n_adler = ro ? 0 : (int32_t)((len + kAdlerPiece - 1) / kAdlerPiece);  // an incremental stream's checksum is its owner's
        pl.n_pieces += s.n_adler;
        pl.w_clear.add(i, (s.out_cap + 65535) / 65536);
        pl.w_adler.add(i, s.n_adler);
        if (s.body_end >= 0 || s.fast_runs > 0 || s.fv_end >= 0)
            pl.w_links.add(i, len - 5 > 0 ? (len - 5 + link_span - 1) / link_span : 0);
        if (s.body_end >= 0) {
            pl.w_match.add(i, (int64_t)s.body_end / kMatchTile + 1);
            pl.w_chunks.add(i, s.nchunks);
            pl.w_segs.add(i, s.nsegs);
            if (s.nsegs > kSupSegs) pl.w_sups.add(i, (s.nsegs + kSupSegs - 1) / kSupSegs);  // shorter streams are resolved row by row
        }
        pl.w_blocks.add(i, s.max_blocks);
        // what none of the parallel forms takes is the one-wave literal engine's: the whole run, not just its last 261 bytes
        if (s.body_end < 0 && s.fv_end < 0 && s.rle_end < 0 && s.fast_runs == 0 && s.plan_nblk == 0 && !(level == 0 && strategy != kRle && !ro)) {
            const int64_t from = resume ? ro->p0 : ro ? ro->hist : 0;
            pl.lit_bytes += std::max<int64_t>(0, len - from - (kMinLookahead - 1));
        }
    }
    {
        // the walk's grids are (most chunks of a stream / 64) x streams: one long stream among thousands of short ones would make
        // them mostly workgroups that return at once, twice per call -- such a batch keeps the maps
        int64_t need = 0;
        for (int i = 0; i < n; i++) need += (pl.sd[(size_t)i].spec_n + 63) / 64;
        if (pl.n_spec && (int64_t)((pl.max_spec_n + 63) / 64) * n > 4 * need + 4096) {
            for (int i = 0; i < n; i++) pl.sd[(size_t)i].spec = 0, pl.sd[(size_t)i].spec_n = 0, pl.sd[(size_t)i].spec_off = 0;
            pl.n_spec = 0, pl.max_spec_n = 0, pl.n_spec_streams = 0;
        }
    }
    return true;
}

// Levels 1-3: every stream's parse as rounds over its chunks, all chunks of the batch at once (zs_fast_sweep.h "Rounds"),
// when that is the shorter way.  One workgroup per stream takes as long as the longest stream at 46 / 35 / 20 MB/s (levels
// 1 / 2 / 3 on text; kennedy.xls and ptt5 are slower).  The rounds take the whole batch through the chip at ~3.5 GB/s a few
// times over and then wait for the last disturbances to die out -- up to ~16 ms on text, less on anything else, and never
// longer than the longest stream takes one workgroup (profiles/r04_fast_batch_shapes.log: 4 x 4 MiB 26 against 88 ms,
// 32 x 4 MiB 46 against 91, 32 x 1 MiB 21 against 23, 64 x 1 MiB 26 against 23, 128 x 256 KiB 10 against 6.6 at level 1; at
// level 3 the rounds win up to 64 x 1 MiB: 31 against 49).
inline void plan_fast_rounds(Plan &pl, const PlanArgs &a, const PlanEnv &env) {
    const int n = a.n, level = a.level;
    int64_t pos_fv = 0, max_fv = 0;
    for (int i = 0; i < n; i++)
        if (pl.sd[(size_t)i].fv_end >= 0) {
            pos_fv += pl.sd[(size_t)i].fv_end + 1 - pl.sd[(size_t)i].start_pos;
            max_fv = std::max<int64_t>(max_fv, pl.sd[(size_t)i].fv_end + 1 - pl.sd[(size_t)i].start_pos);
        }
    const double t_stream = (double)max_fv / (level >= 3 ? 20e6 : level == 2 ? 35e6 : 46e6);
    const double t_rounds = std::min(0.016, (double)max_fv / 60e6) + (double)pos_fv / 3.5e9;
    if (!(env.has_fr_ratio ? (double)pos_fv <= env.fr_ratio * (double)max_fv : t_rounds < t_stream)) return;
    auto one_workgroup_per_stream = [&]() {
        pl.fr_chunks.clear();
        pl.fr_max_n = 0;
        for (int i = 0; i < n; i++) pl.sd[(size_t)i].fr_first = pl.sd[(size_t)i].fr_n = 0;
    };
    int64_t target = plan_fr_target(env, pos_fv);
    bool too_short = false;
    for (;;) {
        pl.fr_chunks.clear();
        pl.fr_max_n = 0;
        too_short = false;
        for (int i = 0; i < n; i++) {
            StreamDesc &s = pl.sd[(size_t)i];
            if (s.fv_end < 0) continue;
            s.fr_first = (int32_t)pl.fr_chunks.size();
            // the stream's read events are its segments (seg_after of event k - 1 = the data end before event k)
            const int32_t *after = pl.seg_after.data() + s.seg_off;
            // (a resumed run: segment 0 is the engine as the flush left it, event 1 the read at p0 itself)
            const bool res = s.resume != 0;
            const int64_t shortest = fs_build_chunks(i, (int64_t)s.fv_end, s.nsegs - 1, [&](int k) { return (int64_t)after[k - 1] - (kMinLookahead - 1); }, (int)target, pl.fr_chunks,
                                                     res ? 2 : 1, res ? s.start_pos : 0);
            if (shortest < kFsMinSpan) too_short = true;  // (Write ends a few hundred bytes apart: more chunks in a chunk's reach than it looks at)
            s.fr_n = (int32_t)pl.fr_chunks.size() - s.fr_first;
            pl.fr_max_n = s.fr_n > pl.fr_max_n ? s.fr_n : pl.fr_max_n;
        }
        if (pl.fr_chunks.size() <= 256 || target >= kFsChunkMax || env.has_fr_chunk) break;
        target += 128;
    }
    if (too_short) one_workgroup_per_stream();
    for (FsChunk &ck : pl.fr_chunks) {
        ck.prov_off = (uint32_t)pl.fr_prov;
        pl.fr_prov += (size_t)(ck.b_hi - ck.b_lo) + kMaxMatch + 64;  // (its loop-tops lie in [b_lo, b_hi + 258))
    }
    if (pl.fr_prov > 0xFFFF0000u) {  // (prov_off is 32 bits: a batch beyond ~4 G positions takes one workgroup per stream)
        one_workgroup_per_stream();
        pl.fr_prov = 0;
    }
}

// The plan of a call: every stream's path and descriptor, the work lists, the parse tables.  The pointers the planner cannot
// know stay null (the tables', ins_bits, the Write table's: plan_bind and the engine) or offsets (plan_blk).  false: `err` says why.
inline bool plan_streams(Plan &pl, const PlanArgs &a, const PlanEnv &env, std::string &err) {
    const LevelCfg lv = level_cfg(a.level);
    // Levels 1-3, a few streams of 256 KiB .. 4 MiB: data that is all period (zeros, image rows, a short period) takes the sweeps'
    // rounds one range a round -- 1 MiB of zeros 57 ms -- and the speculative runs' engine 7; anything else is better off with
    // the sweeps, and which it is the links tell (zs_fast_probe_kernel).  Such a batch is planned for both; the kernels behind
    // the link kernel see the one the probe chose.
    // (a batch with a Write list anywhere is not planned for both: its list-less streams take the sweeps -- the same bytes)
    bool allow_dual = lv.func == 1 && a.strategy != kRle && a.strategy != kHuffmanOnly && !a.any_writes() && !a.ro && !a.rounds && a.force_seq == 0 && !a.force_lit &&
                      a.n <= 16 && !env.no_fast_vec && !env.fast_no_rounds;
    for (int i = 0; i < a.n && allow_dual; i++) allow_dual = a.in_len[i] >= plan_fast_min_input(env) && a.in_len[i] < kFastMinInput;
    // first with the double plan, if the call may have one; then -- a stream the fast forms do not take after all -- the batch
    // as it always was planned
    for (;; allow_dual = false) {
        bool dual_broken = false;
        if (!plan_pass(pl, a, env, allow_dual, dual_broken, err)) return false;
        if (!(allow_dual && dual_broken)) break;
    }
    pl.any_dual = allow_dual;
    if (pl.any_fv && !env.fast_no_rounds && !a.no_rounds && !(a.ro && a.ro->resume && env.no_resume_rounds)) plan_fast_rounds(pl, a, env);
    for (int l = 0; l < kWorkLists; l++) pl.list(l)->finish();
    return true;
}

// Where everything lies.  The descriptors, the work lists' prefixes and the parse tables go back to back into one buffer, as
// they are in the staging area: one copy brings all three (a same-shaped call sends the descriptors alone).  The tables:
// [seg_c0 | seg_after | seg_base | seg_S : int32 x n_segs each][seg_cl : int32 x (n_segs + n)][cstart : int32 x (n_chunks + n)]
// [head : int32 x n_chunks][cl : u32 x n_cl], offsets from the tables' begin.  The work array: list after list.  The Write
// table: every stream's block (zs_core.h write_block_bytes), back to back and 8-byte aligned:
// [ends: int64 x nw][blocks before each Write: int32 x nw][flush modes: u8 x nw]
struct PlanLayout {
    size_t sd_bytes = 0, pre_bytes = 0, geo_bytes = 0, up_bytes = 0;
    size_t o_segcl = 0, o_cstart = 0, o_head = 0, o_cl = 0;
    size_t work[kWorkLists + 1] = {};  // where each list's items begin in the work array; the last: all items
    std::vector<size_t> wr_n, wr_off;  // (a call with Write lists) Writes in each stream's block of the table (0: none) and where it begins
    size_t wr_bytes = 0;
};
inline bool write_block_wanted(const WriteSpec *wr, bool incremental) { return wr && (wr->ends.size() > 1 || wr->flushing() || incremental); }
inline void plan_layout(PlanLayout &lay, const Plan &pl, const PlanArgs &a) {
    const size_t n = (size_t)a.n;
    lay.o_segcl = 16 * (size_t)pl.n_segs, lay.o_cstart = lay.o_segcl + 4 * ((size_t)pl.n_segs + n);
    lay.o_head = lay.o_cstart + 4 * ((size_t)pl.n_chunks + n), lay.o_cl = lay.o_head + 4 * (size_t)pl.n_chunks;
    lay.geo_bytes = lay.o_cl + 4 * pl.cl.size();
    lay.sd_bytes = sizeof(StreamDesc) * n, lay.pre_bytes = 4 * (size_t)kWorkLists * (n + 1);
    lay.up_bytes = lay.sd_bytes + lay.pre_bytes + lay.geo_bytes;
    size_t at = 0;
    for (int l = 0; l < kWorkLists; l++) lay.work[l] = at, at += pl.list(l)->size();
    lay.work[kWorkLists] = at;
    lay.wr_n.clear(), lay.wr_off.clear(), lay.wr_bytes = 0;
    if (a.any_writes()) {
        lay.wr_n.assign(n, 0);
        for (size_t i = 0; i < n; i++)
            if (write_block_wanted(a.writes[i], a.ro != nullptr)) lay.wr_n[i] = a.writes[i]->ends.size();
        lay.wr_bytes = layout_write_blocks(lay.wr_n, lay.wr_off);
    }
}

// The descriptors' pointers into the uploaded buffer (`up`: where its first byte will be), the inserted-position bitmaps
// (one bit per position; pos_off is a multiple of 64: every stream's bitmap starts on a word), the stored-block list and the
// Write table, each null if the plan has none.
inline void plan_bind(Plan &pl, const PlanLayout &lay, const PlanArgs &a, const void *up, uint32_t *ins_bits, const BlockRec *plan_blk, void *wr_table) {
    const uint8_t *gb = (const uint8_t *)up + lay.sd_bytes + lay.pre_bytes;
    const int32_t *g = (const int32_t *)gb;
    for (int i = 0; i < a.n; i++) {
        StreamDesc &s = pl.sd[(size_t)i];
        s.seg_c0 = g + s.seg_off, s.seg_after = g + pl.n_segs + s.seg_off, s.seg_base = g + 2 * pl.n_segs + s.seg_off;
        s.seg_S = g + 3 * pl.n_segs + s.seg_off;
        s.seg_cl = (const int32_t *)(gb + lay.o_segcl) + s.seg_off + i;
        s.cstart = (const int32_t *)(gb + lay.o_cstart) + s.chunk_off + i;
        s.head = (const int32_t *)(gb + lay.o_head) + s.chunk_off;
        s.cl = (const uint32_t *)(gb + lay.o_cl);
        if (ins_bits && s.fv_end >= 0) s.ins_bits = ins_bits + s.pos_off / 32;
        if (plan_blk && s.plan_nblk) s.plan_blk = plan_blk + (uintptr_t)s.plan_blk;
        if (!wr_table || !write_block_wanted(a.writes[i], a.ro != nullptr)) continue;
        const WriteSpec *wr = a.writes[i];
        const size_t nw = lay.wr_n[(size_t)i];
        uint8_t *blk = (uint8_t *)wr_table + lay.wr_off[(size_t)i];
        s.wr_end = (const int64_t *)blk;
        if (wr->flushing() || a.ro) {
            s.wr_blk = (int32_t *)(blk + 8 * nw);
            s.wr_flush = blk + 12 * nw;
        }
    }
}

// The bound plan into the staging area at `hp` (up_bytes): descriptors, the work lists' prefixes (n + 1 each), the tables.
inline void plan_stage(uint8_t *hp, const Plan &pl, const PlanLayout &lay, int n) {
    memcpy(hp, pl.sd.data(), lay.sd_bytes);
    int32_t *hpre = (int32_t *)(hp + lay.sd_bytes);
    for (int l = 0; l < kWorkLists; l++) memcpy(hpre + (size_t)l * (size_t)(n + 1), pl.list(l)->pre.data(), 4 * (size_t)(n + 1));
    if (!lay.geo_bytes) return;
    uint8_t *hg = hp + lay.sd_bytes + lay.pre_bytes;
    if (pl.n_segs) {
        memcpy(hg, pl.seg_c0.data(), 4 * (size_t)pl.n_segs);
        memcpy(hg + 4 * (size_t)pl.n_segs, pl.seg_after.data(), 4 * (size_t)pl.n_segs);
        memcpy(hg + 8 * (size_t)pl.n_segs, pl.seg_base.data(), 4 * (size_t)pl.n_segs);
        memcpy(hg + 12 * (size_t)pl.n_segs, pl.seg_S.data(), 4 * (size_t)pl.n_segs);
    }
    memcpy(hg + lay.o_segcl, pl.seg_cl.data(), 4 * pl.seg_cl.size());
    memcpy(hg + lay.o_cstart, pl.cstart.data(), 4 * pl.cstart.size());
    if (pl.n_chunks) memcpy(hg + lay.o_head, pl.head.data(), 4 * (size_t)pl.n_chunks);
    if (!pl.cl.empty()) memcpy(hg + lay.o_cl, pl.cl.data(), 4 * pl.cl.size());
}
// ... and the Write table (wr_bytes + 64, zeroed by the caller): ends, flush modes, a stored stream's block counts
inline void plan_stage_writes(uint8_t *hw, const Plan &pl, const PlanLayout &lay, const PlanArgs &a) {
    for (int i = 0; i < a.n; i++) {
        const WriteSpec *wr = a.writes[i];
        const size_t nw = lay.wr_n[(size_t)i];
        if (!nw) continue;
        memcpy(hw + lay.wr_off[(size_t)i], wr->ends.data(), sizeof(int64_t) * nw);
        if (wr->flushing() || a.ro) memcpy(hw + lay.wr_off[(size_t)i] + 12 * nw, wr->flush.data(), nw);
        if (!pl.plan_wr_blk.empty()) memcpy(hw + lay.wr_off[(size_t)i] + 8 * nw, pl.plan_wr_blk.data(), 4 * nw);  // (a flushing spec: one stream)
    }
}

}  // namespace zs
