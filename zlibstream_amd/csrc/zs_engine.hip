// zs_engine.hip -- host side of the MI355X deflate engine: workspace, kernel
// pipeline, and the C ABI of include/zsgpu.h (the PNG and CRC-32 calls of it:
// zs_png_host.inc; raw deflate, gzip members and gzip files: zs_wrap_host.inc; ZIP archives: zs_zip_host.inc; TIFF files: zs_tiff_host.inc; OpenEXR files: zs_exr_host.inc; chunked arrays: zs_chunk_host.inc).  No CPU fallback:
// without a usable HIP device every
// compressing entry point fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#define ZS_BUILDING_LIBRARY  // (the test hooks of the header are declared for the library itself)
#include "../../include/zsgpu.h"
#include "zs_kernels.hip"
#include "zs_inflate_par.hip"
#include "zs_inflate_tok.hip"
#include "zs_png.hip"
#include "zs_crc32.hip"
#include "zs_gzip.hip"
#include "zs_zip.hip"
#include "zs_tiff.hip"
#include "zs_exr.hip"
#include "zs_chunk.hip"
#include "zs_plan.h"

using namespace zs;

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

enum Stage {
    kStClear, kStAdler, kStLinks, kStMatch, kStChunkMap, kStSegMap, kStResolve, kStExpand, kStEmitSyms, kStTail, kStTrees,
    kStOffsets, kStEmitBits, kStSpecWalk, kStSpecVerify, kStCrc32, kStSpecCompact, kStPngExpand, kStPngSplit, kStPngPack, kStPngSurvey, kStPngCompose, kStPngDiff, kStPngCrop, kStPart1, kStChunk, kStCount
};
const char *const kStageNames[kStCount] = {"clear", "adler", "links", "match", "chunkmap", "segmap", "resolve", "expand",
                                           "emit_syms", "tail", "trees", "offsets", "emit_bits", "spec_walk", "spec_verify", "crc32_frame",
                                           "spec_compact", "png_expand", "png_split", "png_pack", "png_survey", "png_compose", "png_diff", "png_crop", "part1_chain", "chunk_kn"};

// The context's device buffers of the PNG and CRC-32 calls (zs_png_host.inc), by what they hold: descriptors of a kernel
// (..img, kBufCrcDesc), its records or results, or an intermediate of a call built from several kernels.
enum PngBuf {
    kBufPngImg, kBufPngSeg, kBufPngCtr, kBufPngFimg, kBufPngScratch, kBufPngA7img, kBufPngInflated, kBufPngPasses, kBufCrcDesc, kBufCrcRes, kBufPngZs, kBufPngGather,
    kBufPngXimg, kBufPngRaw, kBufPngSimg, kBufPngSplit, kBufPngGimg, kBufPngVimg, kBufPngVrec, kBufPngPacked, kBufPngCimg, kBufPngFrames, kBufPngDimg, kBufPngDrec,
    kBufPngKimg, kBufPngCrop,
    // the container calls (zs_wrap_host.inc): the members' descriptors and heads, the trailers gathered for the host, the zlib
    // streams in front of the framing launch, a call's files; the ZIP writer's zlib streams (zs_zip_host.inc); the TIFF calls'
    // chunks between inflate or deflate and the predictor kernel, that kernel's descriptors, the writer's zlib streams
    // (zs_tiff_host.inc); the same three of the OpenEXR calls, and KE's segment sums (zs_exr_host.inc); of the chunked-array
    // calls KN's descriptors, the chunks between inflate or deflate and KN, the writer's streams, the survey's records, the
    // chunks between the delta kernels and KN or deflate, the tile records of KL and tile sums of KI (zs_chunk_host.inc)
    kBufWrapHead, kBufWrapGather, kBufWrapZs, kBufWrapFiles, kBufZipZs, kBufTiffChunks, kBufTiffDesc, kBufTiffZs, kBufExrChunks, kBufExrDesc, kBufExrZs, kBufExrSegs,
    kBufChunkDesc, kBufChunkData, kBufChunkZs, kBufChunkRec, kBufChunkDelta, kBufChunkAux,
    kBufPngCount
};

struct PlanCache;  // the last deflate call's plan, kept for a same-shaped call (below, ahead of run_pipeline)

}  // namespace

struct zs_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t aux = nullptr;  // second stream: tree building of the finished blocks runs beside the tail engine
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_pre0 = nullptr, ev_pre = nullptr;
    hipEvent_t ev_spec[4] = {};           // the speculative walk and its verdict; the compaction of its symbols (profiling)
    // the split back end: the symbols in place (main stream), the finished blocks placed (main stream); profiling: the part-1
    // chain on the second stream, from behind the tail engine to its last launch
    hipEvent_t ev_syms = nullptr, ev_part0 = nullptr, ev_part1[2] = {};
    std::string err;
    bool profiling = false;
    int fast_fallbacks = 0;  // speculative DeflateFast batches that had to be redone sequentially
    int round_runs = 0;      // batches with streams in the batched cut rounds (their cuts were not one CU's job)
    int cut_rounds = 0;      // rounds of those
    int lit_fallbacks = 0;   // batches run again with a stream on the literal engine (zs_core.h kMapPoisonBit)
    // the last call's speculative chunk walk (levels 4-9): streams that tried it, those of them that went to the maps after
    // all, and chunks whose guessed entry was wrong
    int spec_streams = 0, spec_fallbacks = 0, spec_wrong_chunks = 0;
    int spec_periodic = 0;  // ... and those of the fallbacks that were never walked: the match kernel's tile count said "periodic"
    // where the first stream of the last deflate call has its parse results (zs_ctx_debug_read)
    int64_t dbg_blk_off = 0, dbg_chunk_off = 0, dbg_nchunks = 0, dbg_spec_n = 0, dbg_n_spec = 0;
    int64_t lit_engine_bytes = 0;  // input bytes parsed by the one-wave literal engine beyond the streams' last 261 (zs_ctx_counter)
    // inflate: compressed bytes each stream of the last call used, trailer included (0: unknown / not ended); and, for a
    // probing call (zs_inflate asking whether the stream's end has arrived), where the block chain ended
    std::vector<int64_t> inf_used;
    int64_t *inf_probe = nullptr;
    int inf_lane_streams = 0;  // streams of the last inflate call whose chain had blocks for the lane decoder (checkpoints, no tokens)
    int inf_wave_streams = 0;  // streams of the last inflate call that the block-parallel pass took and handed on to the one-wave decoder
    int64_t png_segments = 0;  // independent runs of rows the last unfilter call found (zs_png.h png_row_cuts)
    int fast_rounds = 0;  // rounds the last call's DeflateFast took over its chunks (0: one workgroup per stream)
    bool no_rounds_once = false;  // the next plan takes one workgroup per stream (set when the rounds gave up)
    int last_op = 0;  // 0: deflate stages, 1: block-parallel inflate stages, 2: deflate at levels 1-3 (for zs_ctx_stage_name)
    hipEvent_t ev[kStCount + 1] = {};
    double stage_ms[kStCount] = {};
    uint32_t *crc_tab = nullptr;
    DevBuf sd, st, work, link, mm, maps, chunk_far, segmap, supmap, seg_entry, seg_symbase, seg_stale, entry, symbase, stale, syms, blk_end, blk_top, blocks, trees, info, tile_bits, pieces, scratch,
        stage_in, stage_out, wr, inf_desc, inf_state, par_ps, par_st, par_work, par_cbits, par_ccnt, par_surv, par_scnt, par_cands, par_tabs, par_toktabs, par_toks, par_ctoks, par_tokstat, par_tails, par_retry, par_fxtab, par_blocks, par_cells,
        par_windows, par_fail, run_syms, run_bits, run_scratch, run_outs, run_fail, adl_tr, adl_res, plan_blk, ins_bits, mm_bak, cut_pos, cut_bkt, win_groups, win_sg, win_maps, win_entries, persist_bak, resume_flag, rle_tiles, own_in, fr_chunks, fr_meta, fr_planes, fr_prov, fr_base, fr_counters, spec_rec, spec_flags, spec_syms;
    uint32_t *crc32_tab = nullptr;        // KC's tables (zs_crc32.h crc32_fill_tables), made at the first CRC-32 call
    DevBuf png[kBufPngCount];             // the PNG and CRC-32 calls' buffers (PngBuf)
    // profiling: around the launches of one PNG or CRC-32 stage at a time -- whoever records the pair waits for its stream
    // and reads the time before it returns, so no two stages hold it at once
    hipEvent_t ev_png[2] = {};
    bool resume_poisoned = false;  // a resumed run met a read the bulk form does not handle: the caller goes on with the literal engine
    void *pinned = nullptr;
    size_t pinned_cap = 0;
    // the Stream API's pinned input buffer (zs_stream_api.inc InBuf): one deflate stream of the context at a time holds it; `own_in` is
    // that stream's input on the device, sent ahead of its first run
    void *pin_io = nullptr;
    size_t pin_io_cap = 0;
    bool pin_io_busy = false;
    void *pin_out = nullptr;  // ... and an inflate stream's decoded output (OutBuf)
    size_t pin_out_cap = 0;
    bool pin_out_busy = false;
    // The plan of the last deflate call (run_pipeline): its host side in `plan`, its descriptors, work-list prefixes and geometry as
    // they were uploaded in `plan_pin` (pinned; `pinned` is reused inside a call for the verdict and the states), its device side
    // in `sd` (descriptors, prefixes and geometry back to back) and `work`.  plan_gen counts whatever may have written those:
    // every buffer that ensure() moves, every call that plans, device_adlers.  The kept plan serves a call only if the count
    // still is what it was when the plan was kept.
    PlanCache *plan = nullptr;
    void *plan_pin = nullptr;
    size_t plan_pin_cap = 0;
    uint64_t plan_gen = 0;
    int plan_reused = 0;  // the last deflate call took the kept plan (zs_ctx_counter)
    hipEvent_t ev_verdict = nullptr;  // behind the copy of the speculative walk's verdicts: the host waits for it, not for the stream
};

namespace {

bool fail(zs_ctx *c, const char *what, hipError_t e) {
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}
#define ZS_HIP(c, call)                                  \
    do {                                                 \
        hipError_t e_ = (call);                          \
        if (e_ != hipSuccess) return fail(c, #call, e_); \
    } while (0)

bool ensure(zs_ctx *c, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return true;
    c->plan_gen++;  // (a buffer moves: the kept plan's descriptors may point into it)
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    // an eighth of headroom so that a slightly larger batch reuses the buffer; without it when the device is nearly full
    size_t want = bytes + bytes / 8 + 4096;
    if (hipMalloc(&b.p, want) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        want = bytes + 4096;
        if (hipMalloc(&b.p, want) != hipSuccess) {
            (void)hipGetLastError();
            b.p = nullptr;
            char msg[160];
            snprintf(msg, sizeof msg, "workspace: %zu bytes do not fit the device's free memory (the pipeline needs ~17 bytes per input byte: split the batch)", bytes);
            c->err = msg;
            return false;
        }
    }
    b.cap = want;
    return true;
}
bool ensure_plan_pin(zs_ctx *c, size_t bytes) {
    if (bytes <= c->plan_pin_cap) return true;
    if (c->plan_pin) (void)hipHostFree(c->plan_pin);
    c->plan_pin = nullptr;
    c->plan_pin_cap = 0;
    ZS_HIP(c, hipHostMalloc(&c->plan_pin, bytes + bytes / 8 + 4096, hipHostMallocDefault));
    c->plan_pin_cap = bytes + bytes / 8 + 4096;
    return true;
}
bool ensure_pinned(zs_ctx *c, size_t bytes) {
    if (bytes <= c->pinned_cap) return true;
    if (c->pinned) (void)hipHostFree(c->pinned);
    c->pinned = nullptr;
    c->pinned_cap = 0;
    ZS_HIP(c, hipHostMalloc(&c->pinned, bytes + 4096, hipHostMallocDefault));
    c->pinned_cap = bytes + 4096;
    return true;
}

// What a same-shaped call takes over from the call before (zs_plan_key.h): the plan, the places of the work lists in the work
// array, and what else the launches read of the planning.
struct PlanCache {
    PlanKey key, probe;     // the kept plan's key; the current call's
    Plan pl;
    bool valid = false;     // pl, plan_pin, sd and work hold a whole plan that was uploaded ...
    uint64_t gen = 0;       // ... when the context's plan_gen was this
    // a call that uploaded from plan_pin has not been waited for to its end: set at the upload, cleared behind the call's last
    // synchronisation -- a call that leaves early (a HIP error, a workspace that does not fit) leaves it set, and the next call plans
    bool in_flight = false;
    PlanLayout lay;         // where the plan's parts lie in sd, work and the Write table
    // a plan for the sweeps and for the speculative runs at once (Plan::any_dual) as it was before a call struck one of them
    bool dual_saved = false;
    std::vector<StreamDesc> dual_sd;
    std::vector<FsChunk> dual_fr;
    int dual_fr_max_n = 0;
    int64_t dual_n_runs = 0;
};

template <class T>
T *dev(DevBuf &b) {
    return (T *)b.p;
}


// One run of an incremental stream (zs_stream_api.inc; one stream per call): what the planning reads of it (zs_plan.h PlanRun)
// and what the run gives back.
struct RunOpts : PlanRun {
    int64_t end_bits = 0;  // out: stream bit position behind the run's last block or marker
};

// The launch side's switches (DESIGN.md section 8 has the table), read at one place, when a call's DeflateCall is made;
// the planning's are the PlanEnv of the call's key.  Per call, but for the two the table says are read once per process.
struct LaunchEnv {
    bool no_plan_reuse = getenv("ZS_NO_PLAN_REUSE") != nullptr, no_supmap = getenv("ZS_NO_SUPMAP") != nullptr;
    // (ZS_NO_DEFER: every cut on the stream's own CU; ZS_FORCE_ROUNDS: the rounds from the first cut on -- for the tests)
    bool no_defer = getenv("ZS_NO_DEFER") != nullptr, force_rounds = getenv("ZS_FORCE_ROUNDS") != nullptr;
    bool tail_serial = getenv("ZS_TAIL_SERIAL") != nullptr, tail_fork = getenv("ZS_TAIL_FORK") != nullptr, fast_no_probe = getenv("ZS_FAST_NO_PROBE") != nullptr;
    bool no_whole_runs = getenv("ZS_NO_WHOLE_RUNS") != nullptr, whole_runs = getenv("ZS_WHOLE_RUNS") != nullptr;
    bool no_split_backend = getenv("ZS_NO_SPLIT_BACKEND") != nullptr;  // the finished blocks wait for the tail engine like the rest
    bool debug = getenv("ZS_DEBUG") != nullptr, debug_cuts = getenv("ZS_DEBUG_CUTS") != nullptr, debug_fa = getenv("ZS_DEBUG_FA") != nullptr;
    const char *debug_chain = getenv("ZS_DEBUG_CHAIN"), *debug_chain_want = getenv("ZS_DEBUG_CHAIN_WANT");
    int k5_ahead = getenv("ZS_K5_AHEAD") ? atoi(getenv("ZS_K5_AHEAD")) : 1;  // lines the symbol kernel's helper wave asks for ahead of a lane
    // ZS_SPEC_CORRUPT=j: chunk j's recorded guess is spoiled (the tests' way to a failed verification)
    int spec_corrupt = getenv("ZS_SPEC_CORRUPT") ? atoi(getenv("ZS_SPEC_CORRUPT")) : -1;
    // (once per process) where the host's share of a call goes: stderr, microseconds; K9's workgroups per block
    static bool host_times() {
        static const bool v = getenv("ZS_HOST_TIMES") != nullptr;
        return v;
    }
    static const char *eb_tiles() {
        static const char *const v = getenv("ZS_EB_TILES");
        return v;
    }
};
// The switches of the sweeps' rounds, the measurements': read once per process, when the first call takes the rounds.
struct RoundsEnv {
    int max_rounds = getenv("ZS_FR_MAX_ROUNDS") ? atoi(getenv("ZS_FR_MAX_ROUNDS")) : 0;
    int range = getenv("ZS_FR_RANGE") ? std::max(1, atoi(getenv("ZS_FR_RANGE"))) : 0;
    int group = getenv("ZS_FR_GROUP") ? atoi(getenv("ZS_FR_GROUP")) : 4, tail = getenv("ZS_FR_TAIL_RANGE") ? atoi(getenv("ZS_FR_TAIL_RANGE")) : 1;
    bool no_seed = getenv("ZS_FR_NO_SEED") != nullptr, fixed = getenv("ZS_FR_RANGE_FIXED") != nullptr, dbg = getenv("ZS_DEBUG") != nullptr;
    double wake = getenv("ZS_FR_WAKE") ? atof(getenv("ZS_FR_WAKE")) : 4.0;
};

// `writes` (optional): one entry per stream, the Writes of a multi-Write stream (null: the stream is one Write).  A spec whose
// Writes carry a flush mode, and `ro`, are the Stream API's and come with one stream only.
bool run_pipeline(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out, const int64_t *out_cap,
                  int64_t *out_len, int *status, int level, int strategy, int hash_variant, hipStream_t stream,
                  const WriteSpec *const *writes = nullptr, int force_seq = 0, RunOpts *ro = nullptr, bool rounds = false,
                  const std::vector<uint8_t> *force_lit = nullptr);

enum { kWClear, kWAdler, kWLinks, kWMatch, kWChunks, kWSegs, kWSups, kWBlocks, kWRuns };  // the work lists, in Plan::list's order

// The state of one deflate call: its arguments, its switches, the plan it runs on and what the steps of the pipeline hand
// each other.  run_pipeline (below the steps) is the sequence.
struct DeflateCall {
    zs_ctx *const c;
    PlanCache &pc;
    // (pl and lay are the context's, not this call's: a re-entry of run_pipeline plans into them again -- see rerun)
    Plan &pl;
    PlanLayout &lay;
    // run_pipeline's arguments, in its order (level -1 is 6 by now; `writes` with the Rle lists folded once begin() is through)
    int n;
    const void *const *in;
    const int64_t *in_len;
    void *const *out;
    const int64_t *out_cap;
    int64_t *out_len;
    int *status;
    int level, strategy, hash_variant;
    hipStream_t stream;
    const WriteSpec *const *writes;
    int force_seq;
    RunOpts *ro;
    bool rounds;
    const std::vector<uint8_t> *force_lit;
    // (ZS_HOST_TIMES counts from here: the members below are made in this order, so the switches' reads are inside the call's time)
    const std::chrono::steady_clock::time_point ht0 = std::chrono::steady_clock::now();
    LevelCfg lv = level_cfg(level);
    PlanEnv penv = plan_env_read();
    LaunchEnv env;
    FoldedWrites folded;
    PlanArgs pa;
    bool any_writes = false, no_rounds_this_call = false, plan_hit = false, plan_keep = false;
    double ht_plan = 0, ht_launched = 0;
    const StreamDesc *d_sd = nullptr;
    StreamState *d_st = nullptr, *hst = nullptr;
    const uint2 *d_work = nullptr;
    bool prof = false;
    K5Spec k5s{};
    int spec_ok_streams = 0;  // streams whose speculative walk verified: the map kernels skip them (all of them: not launched)
    bool need_maps = true, spec_ran = false;
    bool fork_recorded = false;  // the tail engine's fork has its event already (the speculative path)
    bool tail_late = false, tail_serial = false, use_sup = false;
    bool split = false;  // the finished blocks go through K5b, K7, K8 and K9 beside the tail engine (tails_and_symbols)
    int defer_mode = 0, cut_stride = 0;
    // a step ran the batch again (rerun): the call is over and `answer` is what it returns; a step that failed leaves both false
    bool done = false, answer = false;

    double ht_us() const { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - ht0).count(); }
    const uint2 *work(int list) const { return d_work + lay.work[list]; }
    void mark(int i) {
        if (prof) (void)hipEventRecord(c->ev[i], stream);
    }
    // The batch once more, on another plan: the sweeps after runs that did not verify (force_seq), a stream moved to the literal
    // engine (force_lit), the kernels behind the cut rounds (rounds), a call barred from the sweeps' rounds.  It counts the
    // plan it ends with, so that a stream adds the same to lit_engine_bytes whatever its neighbours made the batch do.
    // The plan and the work-list offsets belong to the context: the re-entry plans into them, so whoever calls this
    // returns at once -- `return rerun(...)` -- and nothing of this call reads pl or lay afterwards.  That has to stay so.
    bool rerun(int force_seq_, bool rounds_, const std::vector<uint8_t> *force_lit_) {
        c->lit_engine_bytes -= pl.lit_bytes;
        done = true;
        return answer = run_pipeline(c, n, in, in_len, out, out_cap, out_len, status, level, strategy, hash_variant, stream, writes, force_seq_, ro, rounds_, force_lit_);
    }
    void launch_tail(hipStream_t on) {
        hipLaunchKernelGGL(zs_tail_kernel, dim3((unsigned)n), dim3(1024), kTailLds, on, d_sd, d_st, dev<uint16_t>(c->link),
                           dev<uint32_t>(c->syms), dev<int32_t>(c->blk_end), dev<int32_t>(c->blk_top), dev<BlockRec>(c->blocks),
                           dev<uint8_t>(c->scratch), c->crc_tab, lv, strategy, hash_variant, level);
    }
    void launch_resolve(int mode, int iter) {
        hipLaunchKernelGGL(zs_resolve_kernel, dim3((unsigned)n), dim3(1024), kResolveLds, stream, d_sd, d_st, dev<uint16_t>(c->link),
                           dev<uint2>(c->mm), dev<uint32_t>(c->maps), dev<uint2>(c->segmap),
                           dev<uint16_t>(c->seg_entry), dev<uint32_t>(c->seg_symbase), dev<uint8_t>(c->stale),
                           dev<uint8_t>(c->seg_stale), c->crc_tab, lv, strategy, hash_variant, 0x7FFFFFFF, 0x7FFFFFFF,
                           use_sup ? dev<uint2>(c->supmap) : (const uint2 *)nullptr, dev<uint16_t>(c->chunk_far), mode, dev<int32_t>(c->cut_pos),
                           dev<uint32_t>(c->cut_bkt), cut_stride, iter);
    }
    // few cuts: 128 workgroups each (every 128th position behind the cut); many: fewer, larger ones
    // (the kernel comes as an argument, not as template parameters of this function: its instantiations then stand where the
    // rounds name them, and the device code keeps its order)
    void launch_cuts_repair(decltype(&zs_cuts_repair_kernel<256, 1>) kernel, unsigned gx, int threads, int max_nc, int iter) {
        hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)std::min(max_nc, 65535), (unsigned)std::min(n, 65535)), dim3((unsigned)threads), kRepairLds, stream,
                           d_sd, d_st, dev<uint16_t>(c->link), dev<uint2>(c->mm), dev<uint8_t>(c->stale), dev<uint8_t>(c->seg_stale),
                           dev<uint16_t>(c->chunk_far), c->crc_tab, lv, hash_variant, dev<int32_t>(c->cut_pos), dev<uint32_t>(c->cut_bkt),
                           cut_stride, iter, n);
    }
    bool begin();            // the arguments, the switches, the key: does the call take the kept plan?
    bool bind_plan();        // the workspace of the plan, and the descriptors' pointers into it
    bool plan_and_upload();  // everything a same-shaped call skips
    bool take_kept_plan();
    void launch_setup();
    bool zero_state();
    bool side_work();
    bool run_cut_rounds();
    bool front();            // links, match, the speculative walk or the maps, resolve
    bool spec_walk();
    bool dual_probe();
    bool fast_sweeps();      // levels 1-3
    bool rle_tiles();
    bool tails_and_symbols();
    bool spec_runs();
    bool blocks_and_bits();
    void debug_dumps();
    void stage_times();
    bool finish();           // poisoned streams, streams for the cut rounds, the results
};

bool DeflateCall::begin() {
    for (int i = 0; i < n; i++) {  // what the caller sees if a HIP call fails before the results are known
        out_len[i] = 0;
        if (status) status[i] = ZS_STREAM_ERROR;
    }
    for (int i = 0; i < n && writes; i++) any_writes = any_writes || writes[i] != nullptr;
    if (any_writes && n > 1)
        for (int i = 0; i < n; i++)
            if (ro || (writes[i] && writes[i]->flushing())) {
                c->err = "flush modes and incremental runs take one stream a call";
                return false;
            }
    // A call of the shape of the one before takes its plan (zs_plan_key.h): nothing below down to the descriptor upload depends
    // on the data.  Left to plan as ever, because what they add to the plan is not the arguments': an incremental run (its
    // state, the chains it imports), the re-entries of this function (force_seq, force_lit, rounds, a call barred from the
    // sweeps' rounds), level 0 (the block list on the device) and Writes under a flush mode (the device counts blocks into their
    // table).  ZS_NO_PLAN_REUSE: every call plans.
    no_rounds_this_call = c->no_rounds_once;
    c->no_rounds_once = false;
    c->fast_rounds = 0;
    c->plan_reused = 0;
    bool flush_any = false;
    for (int i = 0; i < n && any_writes; i++)
        if (const WriteSpec *wr = writes[i]) flush_any = flush_any || wr->flushing() || wr->flush.size() != wr->ends.size();
    plan_keep = !ro && !rounds && !force_lit && !no_rounds_this_call && force_seq == 0 && level != 0 && !flush_any && !env.no_plan_reuse;
    if (plan_keep) {
        plan_key_fill(pc.probe, n, in_len, out_cap, level, strategy, hash_variant, force_seq, ro != nullptr, rounds, force_lit != nullptr, no_rounds_this_call,
                      any_writes ? writes : nullptr, penv);
        plan_hit = pc.valid && pc.gen == c->plan_gen && !pc.in_flight && plan_key_equal(pc.key, pc.probe);
    }
    if (!plan_hit) pc.valid = false, pc.dual_saved = false, c->plan_gen++;  // (this call writes the buffers the kept plan lives in)
    writes = fold_rle_writes(folded, n, in_len, writes, any_writes, level, strategy, ro != nullptr, penv);
    pa.n = n, pa.in = in, pa.in_len = in_len, pa.out = out, pa.out_cap = out_cap, pa.level = level, pa.strategy = strategy;
    pa.writes = writes, pa.force_seq = force_seq, pa.ro = ro, pa.rounds = rounds, pa.force_lit = force_lit, pa.no_rounds = no_rounds_this_call;
    return true;
}

bool DeflateCall::bind_plan() {
    const int spec_bits = plan_spec_bits(penv);
    if (!ensure(c, c->sd, lay.up_bytes + 64) || !ensure(c, c->st, sizeof(StreamState) * (size_t)n) ||
        !ensure(c, c->work, sizeof(uint2) * (lay.work[kWorkLists] + 1)) || !ensure(c, c->link, 2 * (size_t)pl.n_pos + 64) ||
        !ensure(c, c->mm, 8 * (size_t)pl.n_pos + 256) ||  // the symbol kernel stages whole 128-byte lines
        !ensure(c, c->maps, 4 * (size_t)(pl.n_chunks + 1) * kSlots) || !ensure(c, c->segmap, 8 * (size_t)(pl.n_segs + 1) * kSlots) ||
        !ensure(c, c->supmap, 8 * (size_t)(pl.n_sups + 1) * kSlots) || !ensure(c, c->chunk_far, 2 * (size_t)pl.n_chunks + 64) ||
        !ensure(c, c->seg_entry, 2 * (size_t)(pl.n_segs + 2)) || !ensure(c, c->seg_symbase, 4 * (size_t)(pl.n_segs + 2)) ||
        !ensure(c, c->seg_stale, (size_t)pl.n_segs + 64) || !ensure(c, c->entry, 2 * (size_t)(pl.n_chunks + 2)) ||
        !ensure(c, c->symbase, 4 * (size_t)(pl.n_chunks + 2)) || !ensure(c, c->stale, (size_t)pl.n_chunks + 64) ||
        !ensure(c, c->syms, 4 * (size_t)pl.n_syms + kSymsSlack) || !ensure(c, c->blk_end, 4 * (size_t)pl.n_blocks + 64) ||
        !ensure(c, c->blk_top, 4 * (size_t)pl.n_blocks + 64) || !ensure(c, c->blocks, sizeof(BlockRec) * (size_t)pl.n_blocks) ||
        !ensure(c, c->trees, sizeof(TreeWork) * (size_t)pl.n_blocks) || !ensure(c, c->info, sizeof(BlockInfo) * (size_t)pl.n_blocks) ||
        !ensure(c, c->tile_bits, 4 * (size_t)kEbTiles * (size_t)pl.n_blocks + 64) ||
        !ensure(c, c->pieces, 4 * (size_t)pl.n_pieces + 64) || !ensure(c, c->scratch, (size_t)kScratchBytes * (size_t)n) ||
        !ensure(c, c->cut_pos, 8 * (size_t)pl.n_cuts + 64) || !ensure(c, c->cut_bkt, 8 * (size_t)pl.n_cuts + 64) ||
        (pl.n_spec && (!ensure(c, c->spec_rec, 8 * (size_t)pl.n_spec + 64) || !ensure(c, c->spec_flags, 4 * (size_t)n + 64) ||
                       !ensure(c, c->spec_syms, 4 * (size_t)pl.n_spec * (size_t)spec_slab_stride(spec_bits) + 64))))
        return false;
    if (pl.any_fv && !ensure(c, c->ins_bits, (size_t)pl.n_pos / 8 + kFvBitSlack)) return false;
    if (!pl.plan_blk.empty() && !ensure(c, c->plan_blk, sizeof(BlockRec) * pl.plan_blk.size())) return false;
    if (pl.n_runs &&
        (!ensure(c, c->run_syms, 4 * (size_t)pl.n_runs * kFastRunSyms) || !ensure(c, c->run_bits, 4 * (size_t)pl.n_runs * kFastRunBitWords) ||
         !ensure(c, c->run_scratch, (size_t)pl.n_runs * kFastRunScratch) || !ensure(c, c->run_outs, sizeof(FastRunOut) * (size_t)pl.n_runs) ||
         !ensure(c, c->run_fail, 4 * (size_t)n + 64)))
        return false;
    if (any_writes && !ensure(c, c->wr, lay.wr_bytes + 64)) return false;
    plan_bind(pl, lay, pa, c->sd.p, pl.any_fv ? dev<uint32_t>(c->ins_bits) : nullptr, pl.plan_blk.empty() ? nullptr : dev<BlockRec>(c->plan_blk),
              any_writes ? c->wr.p : nullptr);
    return true;
}

bool DeflateCall::plan_and_upload() {
    if (!plan_streams(pl, pa, penv, c->err)) return false;
    plan_layout(lay, pl, pa);
    if (!bind_plan()) return false;
    // rounds: the call goes on behind the batched cut rounds of the call that made it -- same plan, same workspace; nothing
    // is uploaded or zeroed again and the kernels up to the resolve kernel are not run (the descriptors get the pointers
    // into the Write table again: the table itself is on the device already)
    if (any_writes && !rounds && lay.wr_bytes) {
        std::vector<uint8_t> hw(lay.wr_bytes + 64, 0);
        plan_stage_writes(hw.data(), pl, lay, pa);
        ZS_HIP(c, hipMemcpyAsync(c->wr.p, hw.data(), hw.size(), hipMemcpyHostToDevice, stream));
        ZS_HIP(c, hipStreamSynchronize(stream));  // pageable source
    }
    if (!rounds && !pl.plan_blk.empty()) {
        ZS_HIP(c, hipMemcpyAsync(c->plan_blk.p, pl.plan_blk.data(), sizeof(BlockRec) * pl.plan_blk.size(), hipMemcpyHostToDevice, stream));
        ZS_HIP(c, hipStreamSynchronize(stream));  // pageable source
    }
    // ---- upload descriptors, work lists' prefixes and tables: one copy from the plan's own pinned staging area ----
    // (the area keeps them after the call: a same-shaped call puts its pointers into the descriptors there and sends those)
    if (!ensure_pinned(c, std::max(lay.sd_bytes + 16, sizeof(StreamState) * (size_t)n)) || !ensure_plan_pin(c, lay.up_bytes + 16)) return false;
    plan_stage((uint8_t *)c->plan_pin, pl, lay, n);
    if (!rounds) {
        WorkOffsets wo;
        for (int l = 0; l <= kWorkLists; l++) wo.off[l] = (uint32_t)lay.work[l];
        const size_t n_work = lay.work[kWorkLists];
        pc.in_flight = true;
        ZS_HIP(c, hipMemcpyAsync(c->sd.p, c->plan_pin, lay.up_bytes, hipMemcpyHostToDevice, stream));
        if (n_work)
            hipLaunchKernelGGL(zs_worklist_kernel, dim3((unsigned)((n_work + 255) / 256)), dim3(256), 0, stream,
                               (const int32_t *)((const uint8_t *)c->sd.p + lay.sd_bytes), n, wo, dev<uint2>(c->work));
    }
    if (plan_keep) std::swap(pc.key, pc.probe), pc.valid = true, pc.gen = c->plan_gen;
    return true;
}

// the kept plan: the caller's pointers into the kept descriptors, and those alone to the device
bool DeflateCall::take_kept_plan() {
    c->plan_reused = 1;
    if (pc.dual_saved) pl.sd = pc.dual_sd, pl.fr_chunks = pc.dual_fr, pl.fr_max_n = pc.dual_fr_max_n, pl.n_runs = pc.dual_n_runs, pl.any_fv = true;
    StreamDesc *hd = (StreamDesc *)c->plan_pin;
    for (int i = 0; i < n; i++) {
        hd[i].in = pl.sd[(size_t)i].in = (const uint8_t *)in[i];
        hd[i].out = pl.sd[(size_t)i].out = (uint8_t *)out[i];
    }
    pc.in_flight = true;
    ZS_HIP(c, hipMemcpyAsync(c->sd.p, hd, lay.sd_bytes, hipMemcpyHostToDevice, stream));
    return true;
}

void DeflateCall::launch_setup() {
    c->lit_engine_bytes += pl.lit_bytes;
    d_sd = dev<StreamDesc>(c->sd), d_st = dev<StreamState>(c->st), d_work = dev<uint2>(c->work);
    prof = c->profiling;
    c->dbg_blk_off = pl.sd[0].blk_off, c->dbg_chunk_off = pl.sd[0].chunk_off, c->dbg_nchunks = pl.sd[0].nchunks;
    c->dbg_spec_n = pl.sd[0].spec_n, c->dbg_n_spec = pl.n_spec;
    const int spec_bits = plan_spec_bits(penv);
    k5s = K5Spec{dev<uint32_t>(c->spec_rec), dev<uint32_t>(c->spec_rec) + pl.n_spec, spec_bits, plan_spec_warm(penv), env.spec_corrupt,
                 dev<uint32_t>(c->spec_syms), spec_slab_stride(spec_bits)};
    if (!rounds) c->spec_streams = c->spec_fallbacks = c->spec_wrong_chunks = c->spec_periodic = 0;
    const int cut_budget = env.force_rounds ? 0 : kCutBudget;
    defer_mode = ((ro || env.no_defer) ? 0 : 1) | (env.debug_cuts ? 0x100 : 0) | (cut_budget << 16);
    cut_stride = (int)pl.n_cuts;
    use_sup = !pl.w_sups.empty() && !env.no_supmap;
    // the engine is left for a later run, or took the block in progress over from one: it needs K5's symbols and block ends
    tail_late = ro && (!ro->final_run || ro->resume);
    // Beside the symbol kernel the tails of a few streams are free; those of hundreds are not: 256 tail workgroups of 1024
    // threads and 133 KiB of LDS each, one per CU, cost the symbol kernel of 256 x 1 MiB 3 ms (6.8 against 3.9), more than
    // they take alone (0.5).  From 64 streams of 96 KiB or more on the tails run behind the symbols instead (thousands of
    // small streams are the other way round: 16 rounds of tails, a short symbol kernel -- beside each other 18.9 ms for
    // 4096 x 32 KiB, one after the other 20.1).
    // (1024 x 128 KiB: 2.8 ms one after the other, 3.0 side by side; 4096 x 32 KiB: 5.7 against 4.9)
    tail_serial = !tail_late && n >= 64 && (pl.n_pos / n >= (96 << 10) || env.tail_serial) && !env.tail_fork;
}

// The per-run flags and state in one launch (the link array is not cleared: K1 writes every entry that is read).  Launched
// behind K1, which reads none of them -- descriptors, its work items, the input -- and is what the chip waits for at the
// start of a call; the match kernel is the first to touch a stream's state.
bool DeflateCall::zero_state() {
    ZeroRegions z;
    auto reg = [&](int r, DevBuf &b, size_t bytes) {
        z.p[r] = b.p;
        z.n16[r] = (uint32_t)(((bytes + 15) / 16 < b.cap / 16) ? (bytes + 15) / 16 : b.cap / 16);
    };
    reg(0, c->stale, (size_t)pl.n_chunks + 64);
    reg(1, c->seg_stale, (size_t)pl.n_segs + 64);
    reg(2, c->st, sizeof(StreamState) * (size_t)n);
    if (pl.any_fv) reg(3, c->ins_bits, (size_t)pl.n_pos / 8 + kFvBitSlack);
    else z.p[3] = nullptr, z.n16[3] = 0;
    uint32_t most = 0;
    for (int r = 0; r < 4; r++) most = z.n16[r] > most ? z.n16[r] : most;
    unsigned blocks = (most + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(zs_zero_kernel, dim3(blocks), dim3(256), 0, stream, z);
    if (ro && ro->resume && pl.sd[0].fv_end >= 0) {
        // a resumed run at levels 1-3: below p0 the set is what the suspended engine's chains contain -- every position they
        // reach is in it (and no walk meets another one): all ones
        // (exactly the bits below p0: the chunk form's commit ORs the run's own bits in)
        const int64_t lo = std::max<int64_t>(0, ro->p0 - kWSize - 64) / 32, hi = ro->p0 / 32;
        if (hi > lo) ZS_HIP(c, hipMemsetAsync(pl.sd[0].ins_bits + lo, 0xFF, (size_t)(hi - lo) * 4, stream));
        ZS_HIP(c, hipMemsetD32Async((hipDeviceptr_t)(pl.sd[0].ins_bits + hi), (int)((1u << (ro->p0 & 31)) - 1u), 1, stream));
    }
    return true;
}

// the output buffers' clearing and the Adler-32 pieces are wanted by the last two kernels only: they run on the second
// stream beside the link and match kernels (their stages are reported as 0: 0.015 and 0.03 ms on english64 alone, and
// their events are not recorded).  The host enqueues them behind the first launches of the critical path: every call
// in front of K1 is ~5 us in which the device waits for the host.
bool DeflateCall::side_work() {
    ZS_HIP(c, hipStreamWaitEvent(c->aux, c->ev_pre0, 0));
    if (!pl.w_clear.empty())
        hipLaunchKernelGGL(zs_clear_kernel, dim3((unsigned)pl.w_clear.size()), dim3(256), 0, c->aux, d_sd, work(kWClear));
    if (!pl.w_adler.empty())
        hipLaunchKernelGGL(zs_adler_kernel, dim3((unsigned)pl.w_adler.size()), dim3(256), 0, c->aux, d_sd, work(kWAdler),
                           dev<uint32_t>(c->pieces));
    ZS_HIP(c, hipEventRecord(c->ev_pre, c->aux));
    return true;
}

// Batched cut rounds, for the streams the resolve kernel has given up (StreamState::deferred = 1: data whose read events
// are equal-bucket ones by the dozen -- zeros, runs, zero pages -- or with thousands of positions to walk again behind
// each).  Where a cut falls depends on the parse up to it, and the parse on the repairs of the cuts before: one CU doing
// cut, repair, cut, repair is what made such streams 30-170 times slower than text.  Instead: a dry pass of the resolve
// kernel walks the rest of the stream on the records as they are and collects every cut on its way; the records from the
// first cut that differs from the pass before are put back as they were (a copy made when the rounds began) and all
// the cuts of the pass are repaired at once over the chip; the maps of the chunks that changed are made again; and so
// on until a pass finds the cuts of the pass before -- then the records it walked are the ones those cuts leave, which
// is what the one-after-the-other order gives (the first cut never depends on a repair, the second only on the
// first's, ...: a pass fixes at least one more cut, in practice nearly all of them).
bool DeflateCall::run_cut_rounds() {
    // (the records as they are now, and behind them the chunks' largest match distances: what a restore puts back)
    const size_t far_off = 8 * (size_t)pl.n_pos + 256;
    if (!ensure(c, c->mm_bak, far_off + 2 * (size_t)pl.n_chunks + 64)) return false;
    ZS_HIP(c, hipMemcpyAsync(c->mm_bak.p, c->mm.p, 8 * (size_t)pl.n_pos + 256, hipMemcpyDeviceToDevice, stream));
    ZS_HIP(c, hipMemcpyAsync((uint8_t *)c->mm_bak.p + far_off, c->chunk_far.p, 2 * (size_t)pl.n_chunks + 64, hipMemcpyDeviceToDevice, stream));
    ZS_HIP(c, hipMemsetAsync(c->cut_pos.p, 0xFF, 8 * (size_t)pl.n_cuts + 64, stream));  // no cut in any slot (the pass before the first)
    StreamState *hr = (StreamState *)c->pinned;
    for (int iter = 0;; iter++) {
        launch_resolve(3 | (defer_mode & 0x100), iter);
        ZS_HIP(c, hipMemcpyAsync(hr, d_st, sizeof(StreamState) * (size_t)n, hipMemcpyDeviceToHost, stream));
        ZS_HIP(c, hipStreamSynchronize(stream));
        bool all_same = true;
        int max_nc = 0;
        for (int i = 0; i < n; i++)
            if (hr[i].deferred == 1 && !hr[i].cuts_same) all_same = false, max_nc = std::max(max_nc, hr[i].nc[iter & 1]);
        hipLaunchKernelGGL(zs_cuts_apply_kernel, dim3((unsigned)n), dim3(256), 0, stream, d_sd, d_st, dev<uint16_t>(c->link), dev<int32_t>(c->cut_pos),
                           cut_stride, iter);  // (the streams that are through leave the rounds)
        if (env.debug) {
            int nd = 0, nsame = 0;
            for (int i = 0; i < n; i++) nd += hr[i].deferred == 1, nsame += hr[i].deferred == 1 && hr[i].cuts_same;
            fprintf(stderr, "zs: cut round %d: %d streams in the rounds, %d settled, most cuts %d, stream 0: %d cuts, first difference at cut %d (position %d)\n", iter,
                    nd, nsame, max_nc, hr[0].nc[iter & 1], hr[0].cut_diff_idx, hr[0].cut_diff_pos);
        }
        if (all_same && env.debug_cuts) {  // the cuts the rounds settled on, stream 0
            const int ncap = hr[0].nc[iter & 1];
            std::vector<int32_t> cp((size_t)ncap);
            std::vector<uint32_t> cb((size_t)ncap);
            (void)hipMemcpy(cp.data(), dev<int32_t>(c->cut_pos) + (size_t)(iter & 1) * (size_t)cut_stride + pl.sd[0].cut_off, 4 * (size_t)ncap, hipMemcpyDeviceToHost);
            (void)hipMemcpy(cb.data(), dev<uint32_t>(c->cut_bkt) + (size_t)(iter & 1) * (size_t)cut_stride + pl.sd[0].cut_off, 4 * (size_t)ncap, hipMemcpyDeviceToHost);
            fprintf(stderr, "zs: cuts of stream 0 (slot: position / bucket):");
            for (int k = 0; k < ncap; k++)
                if (cp[(size_t)k] >= 0) fprintf(stderr, " %d: %d / %u", k, cp[(size_t)k], cb[(size_t)k]);
            fprintf(stderr, "\n");
        }
        if (all_same) break;
        if (iter >= 4096) {
            c->err = "the cut rounds did not settle";
            return false;
        }
        c->cut_rounds++;
        if (iter > 0)  // (before the first round's repairs the records are the copy)
        hipLaunchKernelGGL(zs_cut_restore_kernel, dim3(2048, (unsigned)std::min(n, 65535)), dim3(256), 0, stream, d_sd, d_st, dev<uint2>(c->mm), (const uint2 *)c->mm_bak.p,
                           dev<uint8_t>(c->stale), dev<uint8_t>(c->seg_stale), dev<uint16_t>(c->chunk_far), (const uint16_t *)((const uint8_t *)c->mm_bak.p + far_off), n);
        if (max_nc > 0) {
            if (max_nc <= 64) launch_cuts_repair(zs_cuts_repair_kernel<256, 1>, 128, 256, max_nc, iter);
            else if (max_nc <= 2048) launch_cuts_repair(zs_cuts_repair_kernel<256, 8>, 16, 256, max_nc, iter);
            else launch_cuts_repair(zs_cuts_repair_kernel<1024, 32>, 1, 1024, max_nc, iter);
        }
        hipLaunchKernelGGL(zs_chunkmap_kernel, dim3((unsigned)pl.w_chunks.size()), dim3(512), 0, stream, d_sd, work(kWChunks),
                           dev<uint2>(c->mm), dev<uint16_t>(c->link), dev<uint32_t>(c->maps), c->crc_tab, lv, strategy,
                           hash_variant, dev<uint16_t>(c->chunk_far), dev<uint8_t>(c->stale), (const StreamState *)d_st);
        hipLaunchKernelGGL(zs_segmap_kernel, dim3((unsigned)pl.w_segs.size()), dim3(320), 0, stream, d_sd, work(kWSegs),
                           dev<uint32_t>(c->maps), dev<uint2>(c->segmap));
        ZS_HIP(c, hipMemsetAsync(c->seg_stale.p, 0, (size_t)pl.n_segs + 64, stream));
        if (use_sup)
            hipLaunchKernelGGL(zs_supmap_kernel, dim3((unsigned)pl.w_sups.size()), dim3(320), 0, stream, d_sd, work(kWSups),
                               dev<uint2>(c->segmap), dev<uint8_t>(c->seg_stale), dev<uint2>(c->supmap));
    }
    return true;
}

// The front of the pipeline, which the re-entry behind the cut rounds skips: links, match search, and the parse's entries -- by
// the speculative walk, or by the maps and the resolve kernel.
bool DeflateCall::front() {
    mark(2);
    if (!pl.w_links.empty())
        hipLaunchKernelGGL(zs_links_kernel, dim3((unsigned)pl.w_links.size()), dim3(1024), kLkLds, stream, d_sd, work(kWLinks),
                           dev<uint16_t>(c->link), c->crc_tab, hash_variant, (int)pl.link_span);
    if (!zero_state()) return false;
    if (ro && ro->resume)
        hipLaunchKernelGGL(zs_import_chains_kernel, dim3(64), dim3(1024), 0, stream, d_sd, 0, dev<uint16_t>(c->link), c->crc_tab, hash_variant, ro->p0);
    if (pl.any_dual && !dual_probe()) return false;
    mark(3);
    if (strategy == kHuffmanOnly) {
        // Longest_match is never called (Deflate.Slow.cs:66-71): every position has no match
        ZS_HIP(c, hipMemsetAsync(c->mm.p, 0, 8 * (size_t)pl.n_pos + 64, stream));
    } else if (!pl.w_match.empty())
        hipLaunchKernelGGL(zs_match_kernel, dim3((unsigned)pl.w_match.size()), dim3(1024), kMatchLds + 16, stream, d_sd, work(kWMatch),
                           dev<uint16_t>(c->link), dev<uint2>(c->mm), lv, strategy, d_st);
    mark(4);
    if (!side_work()) return false;
    if (pl.n_spec && !spec_walk()) return false;
    need_maps = spec_ok_streams < n;
    const StreamState *spec_st = spec_ok_streams ? (const StreamState *)d_st : nullptr;
    if (!pl.w_chunks.empty() && need_maps)
        hipLaunchKernelGGL(zs_chunkmap_kernel, dim3((unsigned)pl.w_chunks.size()), dim3(512), 0, stream, d_sd, work(kWChunks),
                           dev<uint2>(c->mm), dev<uint16_t>(c->link), dev<uint32_t>(c->maps), c->crc_tab, lv, strategy,
                           hash_variant, dev<uint16_t>(c->chunk_far), (uint8_t *)nullptr, (const StreamState *)nullptr, spec_st);
    mark(5);
    if (!pl.w_segs.empty() && need_maps)
        hipLaunchKernelGGL(zs_segmap_kernel, dim3((unsigned)pl.w_segs.size()), dim3(320), 0, stream, d_sd, work(kWSegs),
                           dev<uint32_t>(c->maps), dev<uint2>(c->segmap), spec_st);
    // the segment maps composed 16 at a time, for the resolve kernel's short way through a long stream (ZS_NO_SUPMAP: without)
    if (use_sup && need_maps)
        hipLaunchKernelGGL(zs_supmap_kernel, dim3((unsigned)pl.w_sups.size()), dim3(320), 0, stream, d_sd, work(kWSups),
                           dev<uint2>(c->segmap), dev<uint8_t>(c->seg_stale), dev<uint2>(c->supmap), spec_st);
    mark(6);
    // A stream whose refills are equal-bucket ones with positions to walk again by the thousand (zero pages, runs) is not
    // one CU's job: the resolve kernel gives it up after kDeferBudget such cuts (the kernels behind it skip the stream) and the
    // batch is run again in rounds -- the kernel stops at every such cut, the repair and the chunk maps behind it run over the
    // chip, and the kernel goes on (it keeps its place in StreamState).
    // (Only where a walk is long -- chains of 1024 and 4096, levels 8 and 9: a round costs ~0.1 ms of launches and a
    // synchronisation, which is what a cut's repair takes on one CU at level 6.  64 MiB of short runs: level 9 7.3 s -> 2.0 s,
    // level 6 175 ms inline against 237 in rounds.)
    if (need_maps) launch_resolve(defer_mode, 0);
    return true;
}

// A batch planned for the sweeps and for the speculative runs at once (zs_plan.h plan_streams, allow_dual).  The links are
// there: which is it?  The other plan is struck from the descriptors
bool DeflateCall::dual_probe() {
    bool periodic = true;
    if (!env.fast_no_probe) {
        hipLaunchKernelGGL(zs_fast_probe_kernel, dim3((unsigned)n), dim3(256), 0, stream, d_sd, dev<uint16_t>(c->link), dev<int32_t>(c->run_fail));
        std::vector<int32_t> np((size_t)n, 0);
        ZS_HIP(c, hipMemcpyAsync(np.data(), c->run_fail.p, 4 * (size_t)n, hipMemcpyDeviceToHost, stream));
        ZS_HIP(c, hipStreamSynchronize(stream));
        for (int i = 0; i < n; i++) periodic = periodic && np[(size_t)i] == 0;
    }
    // (a kept plan keeps both: what is struck here is put back when a same-shaped call takes the plan, whose links decide anew)
    if (pc.valid && !pc.dual_saved) pc.dual_saved = true, pc.dual_sd = pl.sd, pc.dual_fr = pl.fr_chunks, pc.dual_fr_max_n = pl.fr_max_n, pc.dual_n_runs = pl.n_runs;
    for (int i = 0; i < n; i++) {
        StreamDesc &sk = pl.sd[(size_t)i];
        if (periodic) sk.fv_end = -1, sk.fr_first = 0, sk.fr_n = 0;
        else sk.fast_runs = 0, sk.run_slots = 0;
    }
    if (periodic) pl.any_fv = false, pl.fr_chunks.clear(), pl.fr_max_n = 0;
    else pl.n_runs = 0;
    memcpy(c->pinned, pl.sd.data(), sizeof(StreamDesc) * (size_t)n);  // (the staging copy's uploads are through: the stream was just waited for)
    ZS_HIP(c, hipMemcpyAsync(c->sd.p, c->pinned, sizeof(StreamDesc) * (size_t)n, hipMemcpyHostToDevice, stream));
    if (env.debug) fprintf(stderr, "zs: %d stream(s) below 4 MiB at level %d: %s\n", n, level, periodic ? "all period, the speculative runs" : "the sweeps");
    return true;
}

// The speculative chunk walk: every chunk of the streams that qualify walked from a guessed entry, the guesses checked
// against the exits, one look at the verdicts.  A stream that verified has its chunks' entries and first symbols and what
// the resolve kernel would leave; the others -- and the streams that never qualified, with no look at anything -- take the maps.
bool DeflateCall::spec_walk() {
    spec_ran = true;
    hipLaunchKernelGGL((zs_emit_syms_lane_kernel<4, 1>), dim3((unsigned)((pl.max_spec_n + 63) / 64), (unsigned)n), dim3(kK5Threads), 0, stream, d_sd, d_st,
                       (const uint2 *)nullptr, 0, dev<uint2>(c->mm), dev<uint16_t>(c->link), (const uint16_t *)nullptr, (const uint32_t *)nullptr,
                       (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, c->crc_tab, lv, strategy, hash_variant, env.k5_ahead, k5s);
    if (prof) (void)hipEventRecord(c->ev_spec[0], stream);
    hipLaunchKernelGGL(zs_spec_verify_kernel, dim3((unsigned)n), dim3(1024), 0, stream, d_sd, d_st, dev<uint2>(c->mm), dev<uint16_t>(c->link), c->crc_tab, lv,
                       strategy, hash_variant, k5s, dev<int32_t>(c->spec_flags));
    int32_t *hf = (int32_t *)c->pinned;  // (the staging copy's uploads are through by the time the verdicts arrive: same stream)
    ZS_HIP(c, hipMemcpyAsync(hf, c->spec_flags.p, 4 * (size_t)n, hipMemcpyDeviceToHost, stream));
    ZS_HIP(c, hipEventRecord(c->ev_verdict, stream));
    // The chip does not wait for the host's look at the verdicts: the compaction of the verified streams' symbols goes in
    // right behind them.  It is predicated on the device (StreamState::spec_ok, per stream), reads only what the walk and the
    // verdict kernel left (records, bases, slabs) and writes only verified streams' symbols and block cuts, none of which the
    // map path of the other streams touches -- so it may run ahead of that path as well as behind it.  The tail engine's
    // fork keeps its place behind the verdict kernel: its event is recorded here, in front of the compaction (a stream that
    // takes the maps records it again behind the resolve kernel, below).
    if (!tail_late && !tail_serial) {
        ZS_HIP(c, hipEventRecord(c->ev_fork, stream));
        fork_recorded = true;
    }
    if (prof) (void)hipEventRecord(c->ev_spec[2], stream);
    hipLaunchKernelGGL(zs_spec_compact_kernel, dim3((unsigned)((pl.max_spec_n + 3) / 4), (unsigned)n), dim3(256), 0, stream, d_sd, d_st, k5s,
                       dev<uint32_t>(c->syms), dev<int32_t>(c->blk_end), dev<int32_t>(c->blk_top));
    if (prof) (void)hipEventRecord(c->ev_spec[3], stream);
    ZS_HIP(c, hipEventSynchronize(c->ev_verdict));
    if (prof) (void)hipEventRecord(c->ev_spec[1], stream);
    for (int i = 0; i < n; i++) {
        if (hf[i] == 0) continue;
        c->spec_streams++;
        if (hf[i] == 1) spec_ok_streams++;
        else c->spec_fallbacks++;
        if (hf[i] == 2) c->spec_periodic++;  // (the verdicts: 1 verified, 2 periodic -- never walked, 3 an event bailed, 4 wrong guesses)
    }
    if (spec_ok_streams < c->spec_streams) {  // how many guesses were wrong: the streams' states (a failed attempt is rare)
        StreamState *hs = (StreamState *)c->pinned;
        ZS_HIP(c, hipMemcpyAsync(hs, d_st, sizeof(StreamState) * (size_t)n, hipMemcpyDeviceToHost, stream));
        ZS_HIP(c, hipStreamSynchronize(stream));
        for (int i = 0; i < n; i++) c->spec_wrong_chunks += hs[i].spec_wrong;
    }
    if (env.debug)
        fprintf(stderr, "zs: speculative walk: %d streams tried, %d verified, %d wrong guesses (chunks of %d, warm-up %d)\n", c->spec_streams, spec_ok_streams,
                c->spec_wrong_chunks, 1 << k5s.len_bits, k5s.warm);
    return true;
}

// Levels 1-3: window-wide sweeps of a workgroup (zs_fast_sweep.hip), one workgroup per stream or, the plan having chunks,
// rounds over the chunks of the streams: every round one workgroup per chunk, until a round changes nothing
bool DeflateCall::fast_sweeps() {
    constexpr int fs_lds = fs_lds_bytes<1024, kFsTile1>();
    if (!pl.fr_chunks.empty()) {
        const size_t nch = pl.fr_chunks.size(), plane_words = (size_t)pl.n_pos / 32 + kFvBitSlack / 4 + 64;
        static const RoundsEnv re;  // the switches of the measurements, read once (not per round)
        const int max_rounds = re.max_rounds ? re.max_rounds : pl.fr_max_n + 2;  // (chunk r of a stream is the reference's after round r at the latest)
        if (!ensure(c, c->fr_chunks, nch * sizeof(FsChunk)) || !ensure(c, c->fr_meta, 2 * nch * sizeof(FsMeta)) || !ensure(c, c->fr_planes, 16 * plane_words) ||
            !ensure(c, c->fr_prov, 4 * pl.fr_prov + 64) || !ensure(c, c->fr_base, 4 * nch + 64) || !ensure(c, c->fr_counters, 4 * ((size_t)max_rounds + 16))) {
            // no room for the rounds' planes and provisional symbols: one workgroup per stream needs none of them
            c->err.clear();
            ZS_HIP(c, hipStreamSynchronize(c->aux));
            ZS_HIP(c, hipStreamSynchronize(stream));
            c->no_rounds_once = true;
            return rerun(force_seq, false, force_lit);
        }
        ZS_HIP(c, hipMemcpyAsync(c->fr_chunks.p, pl.fr_chunks.data(), nch * sizeof(FsChunk), hipMemcpyHostToDevice, stream));
        ZS_HIP(c, hipMemsetAsync(c->fr_counters.p, 0, 4 * ((size_t)max_rounds + 16), stream));
        // more chunks than CUs: a workgroup takes a range of consecutive chunks in turn, every chunk reading what the chunks before
        // it in the range have just left -- within a range the parse is sequential, and the rounds only have to settle what
        // crosses the ranges' ends (1 MiB of text in chunks of 8192: 43 rounds and 27 runs per chunk with ranges of one, 21 and
        // 11.5 with ranges of four, 6 and 3.5 with ranges of sixteen; tests/model mode frounds)
        // A round's ranges are chosen from what the round before changed: while most chunks still change, as many ranges as CUs;
        // once the chunks that will run again fit the chip (a changed chunk wakes the ~4 behind it), one chunk per workgroup --
        // two active chunks of one range would wait for each other.
        // (below two chipfuls of chunks ranges of one: the corpus, 336 chunks of 11 files, 13.9 / 19.1 ms against 16.5 / 23.6)
        const int range_max = re.range ? re.range : nch >= 512 ? (int)((nch + 255) / 256) : 1;
        FsRounds fr{dev<FsChunk>(c->fr_chunks), dev<FsMeta>(c->fr_meta), dev<uint32_t>(c->fr_planes), dev<uint32_t>(c->fr_prov), dev<uint32_t>(c->fr_counters),
                    (int64_t)plane_words, (int)nch, 0, re.no_seed ? 1 : 0, range_max};
        uint32_t changed = 1;
        int r = 0;
        std::string trace;
        while (r < max_rounds && changed) {
            const int g_n = fr.range > 1 ? 1 : re.group;  // rounds between two looks at the counter (ranges of one)
            const unsigned n_wg = (unsigned)((nch + (size_t)fr.range - 1) / (size_t)fr.range);
            for (int g = 0; g < g_n && r < max_rounds; g++, r++) {
                fr.round = r;
                hipLaunchKernelGGL((zs_fast_sweep_kernel<1024, kFsTile1, true>), dim3(n_wg), dim3(1024), fs_lds, stream, d_sd, d_st, dev<uint16_t>(c->link),
                                   dev<uint32_t>(c->syms), dev<int32_t>(c->blk_end), dev<int32_t>(c->blk_top), lv, strategy, fr);
            }
            ZS_HIP(c, hipMemcpyAsync(&changed, dev<uint32_t>(c->fr_counters) + (r - 1), 4, hipMemcpyDeviceToHost, stream));
            ZS_HIP(c, hipStreamSynchronize(stream));
            if (re.dbg) {
                static auto t_last = std::chrono::steady_clock::now();
                const auto t_now = std::chrono::steady_clock::now();
                char b[64];
                snprintf(b, sizeof b, " %u/%d(%.2f)", changed, fr.range, r <= g_n ? 0.0 : std::chrono::duration<double, std::milli>(t_now - t_last).count());
                t_last = t_now;
                trace += b;
            }
            if (!re.fixed) {
                const size_t awake = std::min<size_t>(nch, (size_t)(re.wake * (double)changed));
                fr.range = std::min<int>(range_max, std::max<int>(re.tail, (int)((awake + 255) / 256)));
            }
        }
        c->fast_rounds = r;
        if (re.dbg) fprintf(stderr, "zs: DeflateFast over %zu chunks of %d streams, up to %d to a workgroup: %d rounds (changed/range:%s)\n", nch, n, range_max, r, trace.c_str());
        if (changed) {
            // (cannot happen: chunk r of a stream is the reference's after round r at the latest.  Should it, the batch takes one
            // workgroup per stream instead of failing the call)
            ZS_HIP(c, hipStreamSynchronize(c->aux));
            c->no_rounds_once = true;
            return rerun(force_seq, false, force_lit);
        }
        const FsMeta *mf = dev<FsMeta>(c->fr_meta) + (size_t)((r - 1) & 1) * nch;
        hipLaunchKernelGGL(zs_fast_commit_scan_kernel, dim3((unsigned)n), dim3(1024), 0, stream, d_sd, d_st, mf, dev<int32_t>(c->fr_base));
        hipLaunchKernelGGL(zs_fast_commit_kernel, dim3((unsigned)nch), dim3(256), 0, stream, d_sd, fr, mf, dev<int32_t>(c->fr_base), dev<uint16_t>(c->link),
                           dev<uint32_t>(c->syms), dev<int32_t>(c->blk_end), dev<int32_t>(c->blk_top));
    } else {
        hipLaunchKernelGGL((zs_fast_sweep_kernel<1024, kFsTile1, false>), dim3((unsigned)n), dim3(1024), fs_lds, stream, d_sd, d_st, dev<uint16_t>(c->link),
                           dev<uint32_t>(c->syms), dev<int32_t>(c->blk_end), dev<int32_t>(c->blk_top), lv, strategy, FsRounds());
    }
    return true;
}

// CompressionStrategy.Rle: the body's symbols from the runs of equal bytes (zs_rle.hip), the tail engine behind them
bool DeflateCall::rle_tiles() {
    const size_t nt = (size_t)pl.n_rle_tiles;
    if (!ensure(c, c->rle_tiles, 4 * (4 * nt + (size_t)n) + 256)) return false;
    int32_t *rb = dev<int32_t>(c->rle_tiles);
    RleTiles rt{rb, rb + nt, rb + 2 * nt, rb + 3 * nt, rb + 4 * nt};
    int max_tiles = 0;
    for (int i = 0; i < n; i++)
        if (pl.sd[(size_t)i].rle_end >= 0) max_tiles = std::max(max_tiles, (pl.sd[(size_t)i].rle_end + kMaxMatch + 1 + 4095) / 4096);
    // (a grid's y ends at 65 535: the tile kernels take the streams in slices)
    auto tiles = [&](auto &&launch) {
        for (int s0 = 0; s0 < n; s0 += 65535) launch(dim3((unsigned)((max_tiles + 3) / 4), (unsigned)std::min(n - s0, 65535)), s0);
    };
    tiles([&](dim3 tg, int s0) { hipLaunchKernelGGL(zs_rle_starts_kernel, tg, dim3(256), 0, stream, d_sd, rt, s0); });
    hipLaunchKernelGGL(zs_rle_scan_kernel, dim3((unsigned)n), dim3(1024), 0, stream, d_sd, rt);
    tiles([&](dim3 tg, int s0) {
        hipLaunchKernelGGL(zs_rle_pass_kernel<0>, tg, dim3(256), 0, stream, d_sd, rt, dev<uint32_t>(c->syms), dev<int32_t>(c->blk_end), dev<int32_t>(c->blk_top), s0);
    });
    hipLaunchKernelGGL(zs_rle_sums_kernel, dim3((unsigned)n), dim3(1024), 0, stream, d_sd, d_st, rt);
    tiles([&](dim3 tg, int s0) {
        hipLaunchKernelGGL(zs_rle_pass_kernel<1>, tg, dim3(256), 0, stream, d_sd, rt, dev<uint32_t>(c->syms), dev<int32_t>(c->blk_end), dev<int32_t>(c->blk_top), s0);
    });
    return true;
}

// The tail engine and the symbols of the map path.  The fork: the tail engine (sequential, one workgroup per stream) needs only
// what the resolve kernel left, so it runs on the second stream beside the symbol kernels -- unless the tails are many
// (tail_serial) or need the symbols (tail_late).
bool DeflateCall::tails_and_symbols() {
    // The split back end (zs_kernels.hip stream_body_blocks): with the tail engine forked, the blocks that end inside the body
    // go through K5b, K7, K8 and K9 on the main stream while it runs, and only what it writes follows behind it on the second
    // stream.  Not where the block list is rewritten for the blocks that exist (blocks_and_bits: that needs the tail engine's
    // count), not beside the speculative runs of levels 1-3 (their blocks are made on the main stream, behind this step), and
    // not where no stream is long enough for a finished block (a symbol is at least a byte): those calls keep their order.
    // Nor a call with a stream on the map path: K4b and K5 run beside the tail engine there and take longer than it does (one
    // chunk's chain in K5 is 0.38 ms), so nothing waits for it and the second set of launches is only a cost (0.04 ms of a
    // 64 KiB stream's 1.01; profiles/split_backend.md).  What splits: streams that all verified on the speculative walk, whose
    // compaction is 0.05 ms against the tail engine's 0.26, and the paths that put no kernel beside it (levels 1-3, Rle).
    const bool beside_k5 = need_maps && (!pl.w_segs.empty() || !pl.w_chunks.empty());
    if (!tail_late && !tail_serial && (n < 64 || penv.no_live_list) && !env.no_split_backend && pl.n_runs == 0 && !beside_k5) {
        int64_t longest = 0;
        for (int i = 0; i < n; i++) longest = std::max(longest, in_len[i]);
        split = longest >= kBlockSyms;
    }
    if (!tail_late && !tail_serial) {
        if (!fork_recorded || need_maps) ZS_HIP(c, hipEventRecord(c->ev_fork, stream));  // (behind the resolve kernel, if it ran)
        ZS_HIP(c, hipStreamWaitEvent(c->aux, c->ev_fork, 0));
        launch_tail(c->aux);
        if (split && prof) (void)hipEventRecord(c->ev_part1[0], c->aux);
        if (!split) ZS_HIP(c, hipEventRecord(c->ev_join, c->aux));
    }
    if (!pl.w_segs.empty() && need_maps)
        hipLaunchKernelGGL(zs_expand_kernel, dim3((unsigned)((pl.w_segs.size() + 63) / 64)), dim3(64), 0, stream, d_sd, d_st,
                           work(kWSegs), (int)pl.w_segs.size(), dev<uint2>(c->mm), dev<uint16_t>(c->link),
                           dev<uint32_t>(c->maps), dev<uint16_t>(c->seg_entry), dev<uint32_t>(c->seg_symbase),
                           dev<uint8_t>(c->stale), dev<uint16_t>(c->entry), dev<uint32_t>(c->symbase), c->crc_tab, lv, strategy,
                           hash_variant);
    mark(8);
    if (!pl.w_chunks.empty() && need_maps)
        hipLaunchKernelGGL((zs_emit_syms_lane_kernel<4, 0>), dim3((unsigned)((pl.w_chunks.size() + 63) / 64)), dim3(kK5Threads), 0, stream, d_sd, d_st,
                           work(kWChunks), (int)pl.w_chunks.size(), dev<uint2>(c->mm), dev<uint16_t>(c->link), dev<uint16_t>(c->entry),
                           dev<uint32_t>(c->symbase), dev<uint32_t>(c->syms), dev<int32_t>(c->blk_end), dev<int32_t>(c->blk_top),
                           c->crc_tab, lv, strategy, hash_variant, env.k5_ahead, k5s);
    // the streams whose speculative walk verified: their symbols from the walk's slabs to their places, and the block cuts.
    // (In the re-entry behind the batched cut rounds -- `rounds` -- nothing of the speculative path is launched: the verified
    // streams' symbols and block cuts are those of the call's first pass, which ran to its end for them; the rounds touch only
    // the records and maps of the streams that were given up, nothing zeroes syms / blk_end / blk_top in between, and the map
    // kernels skip the verified streams by StreamState::spec_ok, which the re-entry does not reset either.
    // tests/test_gpu_spec.py test_a_verified_stream_beside_one_in_the_cut_rounds.)
    // (the compaction of their symbols went in behind the verdict kernel, above)
    mark(9);
    auto body_blocks = [&](hipStream_t on, int part) {
        hipLaunchKernelGGL(zs_body_blocks_kernel, dim3((unsigned)n), dim3(256), 0, on, d_sd, d_st, dev<int32_t>(c->blk_end),
                           dev<int32_t>(c->blk_top), dev<BlockRec>(c->blocks), dev<uint32_t>(c->syms), part);
    };
    if (split) {
        // (part 1 of a stream that does not split reads the symbols the main stream has just placed)
        ZS_HIP(c, hipEventRecord(c->ev_syms, stream));
        body_blocks(stream, kPartBody);
        ZS_HIP(c, hipStreamWaitEvent(c->aux, c->ev_syms, 0));
        body_blocks(c->aux, kPartRest);
        return true;
    }
    if (tail_serial) launch_tail(stream);
    else if (!tail_late) ZS_HIP(c, hipStreamWaitEvent(stream, c->ev_join, 0));
    body_blocks(stream, kPartAll);
    if (tail_late) launch_tail(stream);
    return true;
}

// DeflateFast by speculative chunk runs; a run whose hand-over state does not verify sends the batch to the
// sequential engine (the result is the reference's bytes either way)
bool DeflateCall::spec_runs() {
    if (!env.fast_no_probe && force_seq == 0 && !pl.any_dual) {
        // only data that looks periodic is worth the attempt (zs_fast_probe_kernel); anything else goes to the sweeps right away
        hipLaunchKernelGGL(zs_fast_probe_kernel, dim3((unsigned)n), dim3(256), 0, stream, d_sd, dev<uint16_t>(c->link), dev<int32_t>(c->run_fail));
        std::vector<int32_t> np((size_t)n, 0);
        ZS_HIP(c, hipMemcpyAsync(np.data(), c->run_fail.p, 4 * (size_t)n, hipMemcpyDeviceToHost, stream));
        ZS_HIP(c, hipStreamSynchronize(stream));
        for (int i = 0; i < n; i++)
            if (np[(size_t)i]) {
                ZS_HIP(c, hipStreamSynchronize(c->aux));  // (the forked passes read the workspace that is about to be reused)
                return rerun(1, false, force_lit);
            }
    }
    ZS_HIP(c, hipMemsetAsync(c->run_fail.p, 0, 4 * (size_t)n + 64, stream));
    hipLaunchKernelGGL(zs_fast_run_kernel, dim3((unsigned)pl.w_runs.size()), dim3(1024), kFastRunLds, stream, d_sd, work(kWRuns),
                       dev<uint16_t>(c->link), dev<uint32_t>(c->run_syms), dev<uint32_t>(c->run_bits), dev<uint8_t>(c->run_scratch),
                       dev<FastRunOut>(c->run_outs), c->crc_tab, lv, strategy, hash_variant);
    hipLaunchKernelGGL(zs_fast_verify_kernel, dim3((unsigned)pl.w_runs.size()), dim3(256), 0, stream, d_sd, work(kWRuns),
                       dev<uint32_t>(c->run_bits), dev<FastRunOut>(c->run_outs), dev<int32_t>(c->run_fail));
    std::vector<int32_t> rfail((size_t)n, 0);
    ZS_HIP(c, hipMemcpyAsync(rfail.data(), c->run_fail.p, 4 * (size_t)n, hipMemcpyDeviceToHost, stream));
    ZS_HIP(c, hipStreamSynchronize(stream));
    for (int i = 0; i < n; i++)
        if (rfail[(size_t)i]) {
            ZS_HIP(c, hipStreamSynchronize(c->aux));  // the forked tree pass reads the workspace that is about to be reused
            c->fast_fallbacks++;
            std::vector<FastRunOut> outs((size_t)pl.n_runs);
            ZS_HIP(c, hipMemcpy(outs.data(), c->run_outs.p, sizeof(FastRunOut) * outs.size(), hipMemcpyDeviceToHost));
            if (env.debug)
                for (int j = 0; j < pl.sd[(size_t)i].fast_runs; j++) {
                    const FastRunOut &o = outs[(size_t)pl.sd[(size_t)i].run_off + j];
                    fprintf(stderr, "zs: stream %d run %d ok=%d mark=%lld (+%lld syms) end=%lld nsyms=%lld n_ev=%d\n", i, j, o.ok,
                            (long long)o.mark_pos, (long long)o.mark_nsyms, (long long)o.end_pos, (long long)o.nsyms, o.n_ev);
                }
            // Data whose parse does not fall back into step (a period that is no divisor of anything, zeros, 8 KiB rows): the
            // rounds settle one range a round on it -- the stream at one workgroup's 46 / 35 / 20 MB/s -- while one run of
            // the engine over the whole stream costs ~1 us a symbol, and the runs have just counted the symbols: 5 MiB of a
            // 7-byte period is 20 K matches, 20 ms against 375; ptt5 nine times over is 600 K symbols, 600 ms against 53.  One run per
            // stream when that is the shorter way for the batch by a margin (both are estimates).
            double t_engine = 0, t_sweeps = 0;
            for (int k = 0; k < n; k++) {
                const StreamDesc &sk = pl.sd[(size_t)k];
                if (sk.fast_runs <= 0) continue;
                // (a run's warm-up is a fifth of it: the counts of whole runs, scaled)
                int64_t syms = 0, matches = 0;
                for (int j = 0; j < sk.fast_runs; j++) syms += outs[(size_t)sk.run_off + j].nsyms, matches += outs[(size_t)sk.run_off + j].n_match;
                const double scale = sk.fast_runs > 1 ? 0.8 : 1.0;
                const double te = scale * (1.2e-6 * (double)matches + 0.03e-6 * (double)(syms - matches)) + (double)sk.n / 1.5e9;
                if (env.debug) fprintf(stderr, "zs: stream %d: ~%.0f symbols one at a time, ~%.0f in runs of literals, %d bytes\n", k, scale * (double)matches, scale * (double)(syms - matches), sk.n);
                t_engine = std::max(t_engine, te);
                t_sweeps = std::max(t_sweeps, (double)sk.n / (level >= 3 ? 20e6 : level == 2 ? 35e6 : 46e6));
            }
            const int mode = (force_seq == 0 && !env.no_whole_runs && (env.whole_runs || t_engine < 0.7 * t_sweeps)) ? 2 : 1;
            if (env.debug) fprintf(stderr, "zs: the runs did not verify: %s (engine %.1f ms, sweeps up to %.1f ms)\n", mode == 2 ? "one run per stream" : "the sweeps", t_engine * 1e3, t_sweeps * 1e3);
            return rerun(mode, false, force_lit);
        }
    hipLaunchKernelGGL(zs_fast_plan_kernel, dim3((unsigned)n), dim3(256), 0, stream, d_sd, d_st, dev<FastRunOut>(c->run_outs), n);
    hipLaunchKernelGGL(zs_fast_stitch_kernel, dim3((unsigned)pl.w_runs.size()), dim3(256), 0, stream, d_sd, work(kWRuns),
                       dev<uint32_t>(c->run_syms), dev<FastRunOut>(c->run_outs), dev<uint32_t>(c->syms), dev<int32_t>(c->blk_end),
                       dev<int32_t>(c->blk_top));
    hipLaunchKernelGGL(zs_fast_blocks_kernel, dim3((unsigned)n), dim3(64), 0, stream, d_sd, d_st, dev<FastRunOut>(c->run_outs),
                       dev<int32_t>(c->blk_end), dev<int32_t>(c->blk_top), dev<BlockRec>(c->blocks), n);
    return true;
}

// Blocks to bits: the trees, the blocks' places in the output, the bits; then the wait for the streams' states.
bool DeflateCall::blocks_and_bits() {
    // the tree kernel is one latency chain per block: many small blocks (a batch of small streams) want more resident
    // workgroups, a long stream's 16 Ki-symbol blocks a wider histogram
    const int trees_threads = pl.w_blocks.size() > 8192 ? 128 : 256;
    if (n >= 64 && !penv.no_live_list) {
        // many streams: the block list rewritten with the blocks that exist in front (zs_live_scan_kernel)
        // (its prefix sum goes where the work lists' prefixes were uploaded: zs_worklist_kernel is through with them, and a call
        // that takes this plan over does not run it)
        int32_t *const d_live = (int32_t *)((uint8_t *)c->sd.p + lay.sd_bytes);
        hipLaunchKernelGGL(zs_live_scan_kernel, dim3(1), dim3(1024), 0, stream, d_st, n, d_live);
        hipLaunchKernelGGL(zs_live_fill_kernel, dim3((unsigned)((pl.w_blocks.size() + 255) / 256)), dim3(256), 0, stream, d_live, n,
                           (uint32_t)pl.w_blocks.size(), dev<uint2>(c->work) + lay.work[kWBlocks]);
    }
    auto trees = [&](hipStream_t on, int part) {
        hipLaunchKernelGGL(zs_trees_kernel, dim3((unsigned)pl.w_blocks.size()), dim3(trees_threads), 0, on, d_sd, d_st, work(kWBlocks), dev<uint32_t>(c->syms),
                           dev<BlockRec>(c->blocks), dev<TreeWork>(c->trees), dev<BlockInfo>(c->info), dev<int32_t>(c->tile_bits), strategy, level, part);
    };
    auto offsets = [&](hipStream_t on, int part) {
        hipLaunchKernelGGL(zs_offsets_kernel, dim3((unsigned)n), dim3(256), 0, on, d_sd, d_st, dev<BlockRec>(c->blocks), dev<BlockInfo>(c->info),
                           dev<TreeWork>(c->trees), dev<uint32_t>(c->pieces), level, n, part);
    };
    trees(stream, split ? kPartBody : kPartAll);
    mark(11);
    ZS_HIP(c, hipStreamWaitEvent(stream, c->ev_pre, 0));  // the cleared output and the Adler pieces (second stream, above)
    offsets(stream, split ? kPartBody : kPartAll);
    mark(12);
    if (split) ZS_HIP(c, hipEventRecord(c->ev_part0, stream));  // the finished blocks are placed: part 1 goes on from their end
    // one workgroup for a block's header and one for each of its tiles of symbols, whose bit counts the tree kernel left
    // (a workgroup takes every eb_tiles-th tile: any number covers them all); a symbol is at least one input byte
    int eb_tiles = kEbTiles;
    if (level != 0) {
        int64_t longest = 0;
        for (int i = 0; i < n; i++) longest = std::max(longest, in_len[i]);
        eb_tiles = (int)std::min<int64_t>(kEbTiles, (longest + 1) / kEbTile + 1);
    }
    if (env.eb_tiles()) eb_tiles = std::max(1, std::min(kEbTiles, atoi(env.eb_tiles())));
    auto emit_bits = [&](hipStream_t on, int part) {
        hipLaunchKernelGGL(zs_emit_bits_kernel, dim3((unsigned)pl.w_blocks.size(), (unsigned)(1 + eb_tiles)), dim3(256), 0, on, d_sd, d_st, work(kWBlocks),
                           dev<uint32_t>(c->syms), dev<BlockRec>(c->blocks), dev<TreeWork>(c->trees), dev<BlockInfo>(c->info), dev<int32_t>(c->tile_bits), part);
    };
    emit_bits(stream, split ? kPartBody : kPartAll);
    mark(13);
    if (split) {
        // behind the tail engine and part 1 of K5b (tails_and_symbols): what the tail engine wrote, and every stream that does
        // not split.  The parts of a stream meet in shared output words through atomicOr, like the parts of a block.
        trees(c->aux, kPartRest);
        ZS_HIP(c, hipStreamWaitEvent(c->aux, c->ev_part0, 0));
        offsets(c->aux, kPartRest);
        emit_bits(c->aux, kPartRest);
        if (prof) (void)hipEventRecord(c->ev_part1[1], c->aux);
        ZS_HIP(c, hipEventRecord(c->ev_join, c->aux));
        ZS_HIP(c, hipStreamWaitEvent(stream, c->ev_join, 0));
    }
    ZS_HIP(c, hipGetLastError());
    hst = (StreamState *)c->pinned;
    ZS_HIP(c, hipMemcpyAsync(hst, d_st, sizeof(StreamState) * (size_t)n, hipMemcpyDeviceToHost, stream));
    ht_launched = ht_us();
    ZS_HIP(c, hipStreamSynchronize(stream));
    pc.in_flight = false;
    // (what this call itself moved behind its plan -- the sweeps' rounds, the Rle tiles: buffers the launches take from the
    // context, not from the descriptors -- does not cost the plan it has just made)
    if (pc.valid && !plan_hit) pc.gen = c->plan_gen;
    if (env.host_times())
        fprintf(stderr, "zs: host: plan + uploads %.0f us%s, all launched at %.0f us, device done at %.0f us\n", ht_plan, c->plan_reused ? " (kept plan)" : "", ht_launched,
                ht_us());
    c->last_op = lv.func == 1 ? 2 : 0;
    return true;
}

void DeflateCall::debug_dumps() {
    if (env.debug_chain && n == 1) {  // the chain of one position as the kernels saw it (buffer positions)
        const int64_t q0 = atoll(env.debug_chain) - (ro ? ro->abs_off : 0);
        if (q0 > 0 && q0 < in_len[0]) {
            std::vector<uint16_t> lk((size_t)in_len[0]);
            (void)hipMemcpy(lk.data(), dev<uint16_t>(c->link) + pl.sd[0].pos_off, 2 * (size_t)in_len[0], hipMemcpyDeviceToHost);
            fprintf(stderr, "[zs] run of %lld bytes (stream position %lld on), resume %d at %lld: chain of %lld:", (long long)in_len[0], (long long)(ro ? ro->abs_off : 0),
                    pl.sd[0].resume, (long long)pl.sd[0].start_pos, (long long)q0);
            int64_t q = q0;
            int hops = 0;
            const int64_t want = env.debug_chain_want ? atoll(env.debug_chain_want) - (ro ? ro->abs_off : 0) : -1;
            int want_at = -1;
            while (lk[(size_t)q] && hops < 100000) {
                q -= lk[(size_t)q], hops++;
                if (hops <= 12) fprintf(stderr, " %lld", (long long)q);
                if (q == want) want_at = hops;
            }
            fprintf(stderr, " ... %d hops, ends at %lld; position %lld is hop %d\n", hops, (long long)q, (long long)want, want_at);
        }
    }
    if (env.debug_fa && writes && writes[0] && pl.sd[0].wr_blk) {  // the flush accounting's inputs: blocks flushed before each Write began
        const WriteSpec *wr = writes[0];
        const size_t nw = wr->ends.size();
        std::vector<int32_t> wb(nw);
        (void)hipMemcpy(wb.data(), pl.sd[0].wr_blk, 4 * nw, hipMemcpyDeviceToHost);
        fprintf(stderr, "[zs] run of %lld bytes, %zu Writes, %d blocks, body ends at %d, resume %d; blocks before each Write:", (long long)in_len[0], nw, hst[0].nblocks,
                pl.sd[0].body_end, pl.sd[0].resume);
        for (size_t k = 0; k < nw && k < 24; k++) fprintf(stderr, " %d(end %lld, flush %d)", wb[k], (long long)wr->ends[k], wr->flush.empty() ? 0 : wr->flush[k]);
        fprintf(stderr, "\n");
    }
}

// profiling: the stages' times from the events the steps recorded
void DeflateCall::stage_times() {
    for (int i = 0; i < kStCount; i++) {
        float ms = 0;
        if (i >= kStLinks && i <= kStEmitBits) (void)hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]);  // clear / adler: beside the others, unmarked
        c->stage_ms[i] = ms;
    }
    if (split) {
        // the back end split: trees, offsets and emit_bits above are the part-0 launches, this is the chain behind the tail
        // engine on the second stream, beside them -- the stages of such a call do not sum to its path
        float p1 = 0;
        (void)hipEventElapsedTime(&p1, c->ev_part1[0], c->ev_part1[1]);
        c->stage_ms[kStPart1] = p1;
    }
    if (spec_ran) {  // the speculative walk and its verdict sit between the match kernel and the maps
        float a = 0, b = 0, m = 0;
        (void)hipEventElapsedTime(&a, c->ev[kStChunkMap], c->ev_spec[0]);
        (void)hipEventElapsedTime(&b, c->ev_spec[0], c->ev_spec[1]);
        (void)hipEventElapsedTime(&m, c->ev_spec[1], c->ev[kStChunkMap + 1]);
        c->stage_ms[kStSpecWalk] = a, c->stage_ms[kStSpecVerify] = b, c->stage_ms[kStChunkMap] = m;
        // (the compaction runs inside the verdict's interval, while the host looks at the verdicts: its own share of it)
        float k = 0;
        (void)hipEventElapsedTime(&k, c->ev_spec[2], c->ev_spec[3]);
        c->stage_ms[kStSpecCompact] = k;
        c->stage_ms[kStSpecVerify] = b > k ? b - k : 0;
    }
}

// What the streams' states say: a poisoned stream or one for the cut rounds has the batch run again; else the results.
bool DeflateCall::finish() {
    {
        // a stream whose true path met a read the bulk form does not handle (zs_core.h kMapPoisonBit): the batch again with
        // those streams on the literal engine
        bool any_poison = false;
        std::vector<uint8_t> fl(force_lit ? *force_lit : std::vector<uint8_t>((size_t)n, 0));
        for (int i = 0; i < n; i++)
            if (hst[i].poison) any_poison = true, fl[(size_t)i] = 1;
        if (any_poison) {
            ZS_HIP(c, hipStreamSynchronize(c->aux));
            if (ro && ro->resume) {  // (the engine's state in `persist` has been run over: the caller has kept a copy)
                c->err = "the resumed run met a read the bulk pipeline leaves to the literal engine";
                c->resume_poisoned = true;
                return false;
            }
            c->lit_fallbacks++;
            return rerun(force_seq, false, &fl);
        }
    }
    if (!ro && !rounds) {
        // streams the resolve kernel gave up (zs_device.h, StreamState::deferred): the batched cut rounds, then the kernels
        // behind the resolve kernel once more (they skipped those streams): this call again, from there
        bool gave_up = false;
        for (int i = 0; i < n; i++) gave_up = gave_up || hst[i].deferred == 1;
        if (gave_up) {
            ZS_HIP(c, hipStreamSynchronize(c->aux));
            c->round_runs++;
            if (!run_cut_rounds()) return false;
            return rerun(force_seq, true, force_lit);
        }
    }
    if (ro) ro->end_bits = hst[0].end_bits;
    // every stream's length and code are reported; the first failing one sets the message and the return value
    bool all_ok = true;
    for (int i = 0; i < n; i++) {
        out_len[i] = hst[i].out_len;
        if (status) status[i] = hst[i].status;
        if (hst[i].status != 0 && all_ok) {
            c->err = hst[i].status == ZS_BUF_ERROR ? "buffer error"
                                                   : "stored block larger than the reference's pending buffer (the managed engine throws here)";
            all_ok = false;
        }
    }
    return all_ok;
}

// A deflate call, step by step.  A step that fails returns false; one that ran the batch again (DeflateCall::rerun) has the
// call's answer already.  Nothing here moves a launch, a copy, an event or a synchronisation against another.
bool run_pipeline(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out, const int64_t *out_cap, int64_t *out_len, int *status, int level,
                  int strategy, int hash_variant, hipStream_t stream, const WriteSpec *const *writes, int force_seq, RunOpts *ro, bool rounds,
                  const std::vector<uint8_t> *force_lit) {
    if (!c->plan) c->plan = new PlanCache();
    PlanCache &pc = *c->plan;
    DeflateCall k{c, pc, pc.pl, pc.lay, n, in, in_len, out, out_cap, out_len, status, level == -1 ? 6 : level, strategy, hash_variant, stream, writes, force_seq, ro, rounds, force_lit};
    if (!k.begin()) return false;
    if (!(k.plan_hit ? k.take_kept_plan() : k.plan_and_upload())) return false;
    k.launch_setup();
    k.ht_plan = k.ht_us();
    ZS_HIP(c, hipEventRecord(c->ev_pre0, stream));
    if (!rounds && !k.front()) return false;  // (K1 first: every call in front of it is ~5 us in which the device waits for the host)
    k.mark(7);
    if (k.pl.any_fv && (!k.fast_sweeps() || k.done)) return k.answer;
    if (k.pl.any_rle && !k.rle_tiles()) return false;
    if (!k.tails_and_symbols()) return false;
    if (k.pl.n_runs && (!k.spec_runs() || k.done)) return k.answer;
    k.mark(10);
    if (!k.blocks_and_bits()) return false;
    k.debug_dumps();
    if (k.prof) k.stage_times();
    return k.finish();
}

// Adler-32 (seed 1) of m device buffers in one pass: the piece kernel over all of them, one combining workgroup per
// buffer, one copy back.  `trailers` (optional, device pointers or null entries): the 4 big-endian bytes each result is
// compared with (the check of Inflate.cs:300-345); ok[i] = 1 when they agree.
bool device_adlers(zs_ctx *c, int m, const void *const *bufs, const int64_t *lens, const void *const *trailers, uint32_t *adlers,
                   int *ok, hipStream_t stream) {
    if (m <= 0) return true;
    c->plan_gen++;  // (the descriptors and work items below go where the kept deflate plan has its own)
    std::vector<StreamDesc> sd((size_t)m);
    std::vector<uint2> work;
    int64_t n_pieces = 0;
    for (int i = 0; i < m; i++) {
        StreamDesc &s = sd[(size_t)i];
        memset(&s, 0, sizeof s);
        s.in = (const uint8_t *)bufs[i];
        s.n = (int32_t)lens[i];
        s.adler_off = (int32_t)n_pieces;
        s.n_adler = (int32_t)((lens[i] + kAdlerPiece - 1) / kAdlerPiece);
        n_pieces += s.n_adler;
        for (int k = 0; k < s.n_adler; k++) work.push_back(make_uint2((unsigned)i, (unsigned)k));
    }
    const size_t b_sd = sizeof(StreamDesc) * (size_t)m, b_work = sizeof(uint2) * work.size(), b_tr = sizeof(void *) * (size_t)m;
    if (!ensure(c, c->sd, b_sd) || !ensure(c, c->work, b_work + 16) || !ensure(c, c->pieces, 4 * (size_t)n_pieces + 64) ||
        !ensure(c, c->adl_tr, b_tr) || !ensure(c, c->adl_res, sizeof(uint2) * (size_t)m) ||
        !ensure_pinned(c, b_sd + b_work + b_tr + sizeof(uint2) * (size_t)m))
        return false;
    uint8_t *hp = (uint8_t *)c->pinned;
    memcpy(hp, sd.data(), b_sd);
    if (b_work) memcpy(hp + b_sd, work.data(), b_work);
    if (trailers) memcpy(hp + b_sd + b_work, trailers, b_tr);
    ZS_HIP(c, hipMemcpyAsync(c->sd.p, hp, b_sd, hipMemcpyHostToDevice, stream));
    if (b_work) ZS_HIP(c, hipMemcpyAsync(c->work.p, hp + b_sd, b_work, hipMemcpyHostToDevice, stream));
    if (trailers) ZS_HIP(c, hipMemcpyAsync(c->adl_tr.p, hp + b_sd + b_work, b_tr, hipMemcpyHostToDevice, stream));
    if (!work.empty())
        hipLaunchKernelGGL(zs_adler_kernel, dim3((unsigned)work.size()), dim3(256), 0, stream, dev<StreamDesc>(c->sd), dev<uint2>(c->work),
                           dev<uint32_t>(c->pieces));
    hipLaunchKernelGGL(zs_adler_finish_kernel, dim3((unsigned)m), dim3(256), 0, stream, dev<StreamDesc>(c->sd), dev<uint32_t>(c->pieces),
                       trailers ? (const uint8_t *const *)c->adl_tr.p : nullptr, dev<uint2>(c->adl_res));
    uint2 *hres = (uint2 *)(hp + b_sd + b_work + b_tr);
    ZS_HIP(c, hipMemcpyAsync(hres, c->adl_res.p, sizeof(uint2) * (size_t)m, hipMemcpyDeviceToHost, stream));
    ZS_HIP(c, hipStreamSynchronize(stream));
    for (int i = 0; i < m; i++) {
        if (adlers) adlers[i] = hres[i].x;
        if (ok) ok[i] = (int)hres[i].y;
    }
    return true;
}

// The longest run of streams from `lo` on whose device memory -- per input byte: `per_byte` bytes of workspace (and staging),
// plus the output capacity when it is staged -- fits what the device has free now plus what the context already holds (its
// buffers are reused); at least one stream.
int batch_prefix_that_fits(zs_ctx *c, int n, const int64_t *in_len, const int64_t *out_cap, int lo, int per_byte) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return n;
    const DevBuf *held[] = {&c->link, &c->mm, &c->maps, &c->segmap, &c->supmap, &c->syms, &c->trees, &c->blocks, &c->info, &c->tile_bits, &c->stage_in, &c->stage_out,
                            &c->scratch, &c->ins_bits, &c->mm_bak};
    size_t have = 0;
    for (const DevBuf *b : held) have += b->cap;
    const double budget = 0.55 * ((double)free_b + (double)have);  // (the buffers are grown with an eighth of headroom each)
    double need = 0;
    int hi = lo;
    while (hi < n) {
        const double add = (double)in_len[hi] * per_byte + (per_byte > 19 ? (double)out_cap[hi] : 0.0) + 4.0e6;
        if (hi > lo && need + add > budget) break;
        need += add;
        hi++;
    }
    return hi;
}

bool check_args(zs_ctx *c, int n, const int64_t *in_len, int level, int strategy) {
    if (!c) return false;
    if (n < 0 || level < -1 || level > 9 || strategy < 0 || strategy > 4) {
        c->err = "stream error";
        return false;
    }
    for (int i = 0; i < n; i++)
        if (in_len[i] < 0 || in_len[i] > 0x7FFFFFFF - 1024) {
            c->err = "stream error";
            return false;
        }
    return true;
}

}  // namespace

extern "C" {

void zs_ctx_destroy(zs_ctx *c);
int zs_ctx_create(int device, zs_ctx **out) {
    if (!out) return ZS_STREAM_ERROR;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return ZS_STREAM_ERROR;
    if (hipSetDevice(device) != hipSuccess) return ZS_STREAM_ERROR;
    zs_ctx *c = new zs_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        zs_ctx_destroy(c);  // releases whatever was created so far
        return ZS_MEM_ERROR;
    }
    for (auto &e : c->ev) (void)hipEventCreate(&e);
    for (auto &e : c->ev_spec) (void)hipEventCreate(&e);
    for (auto &e : c->ev_part1) (void)hipEventCreate(&e);
    for (auto &e : c->ev_png) (void)hipEventCreate(&e);
    {
        // the link kernel relies on the LDS applying the lanes of one DS_MSKOR_RTN_B32 in lane order: check it here
        int *d_ok = nullptr, ok = 0;
        if (hipMalloc((void **)&d_ok, sizeof(int)) != hipSuccess) {
            zs_ctx_destroy(c);  // releases whatever was created so far
            return ZS_MEM_ERROR;
        }
        hipLaunchKernelGGL(zs_lds_order_kernel, dim3(1), dim3(64), 0, c->stream, d_ok);
        const bool copied = hipMemcpyAsync(&ok, d_ok, sizeof(int), hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                            hipStreamSynchronize(c->stream) == hipSuccess;
        (void)hipFree(d_ok);
        if (!copied || !ok) {
            fprintf(stderr, "zsgpu: LDS lane-order self-test failed on device %d; this build cannot run there\n", device);
            zs_ctx_destroy(c);
            return ZS_STREAM_ERROR;
        }
    }
    if (hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_pre0, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_pre, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_syms, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_part0, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_verdict, hipEventDisableTiming) != hipSuccess) {
        zs_ctx_destroy(c);  // releases whatever was created so far
        return ZS_MEM_ERROR;
    }
    std::vector<uint32_t> tab(1024);
    for (int t = 0; t < 4; t++)
        for (int i = 0; i < 256; i++) tab[(size_t)t * 256 + i] = crc32c_table_entry(t, (uint32_t)i);
    if (hipMalloc((void **)&c->crc_tab, 4096) != hipSuccess ||
        hipMemcpy(c->crc_tab, tab.data(), 4096, hipMemcpyHostToDevice) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_match_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMatchLds + 16) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_resolve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kResolveLds) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_links_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLkLds) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_tail_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kTailLds) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_fast_run_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kFastRunLds) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_fast_sweep_kernel<1024, kFsTile1, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (fs_lds_bytes<1024, kFsTile1>())) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_fast_sweep_kernel<1024, kFsTile1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (fs_lds_bytes<1024, kFsTile1>())) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_inf_window_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kWinMapLds) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_inf_chain_par_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kChainParLds) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_inf_expand_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kExpLds) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_cuts_repair_kernel<256, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, kRepairLds) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_cuts_repair_kernel<256, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, kRepairLds) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_cuts_repair_kernel<1024, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, kRepairLds) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_png_unfilter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kPngMaxLds) != hipSuccess ||
        hipFuncSetAttribute((const void *)zs_inflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kInfLds) != hipSuccess) {
        zs_ctx_destroy(c);
        return ZS_MEM_ERROR;
    }
    // the match kernel addresses its tile from LDS address 0 (lds0_u32 ...): true as long as it has no static LDS
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, (const void *)zs_match_kernel) != hipSuccess || fa.sharedSizeBytes != 0) {
        fprintf(stderr, "zsgpu: zs_match_kernel has static LDS; its tile addressing assumes none\n");
        zs_ctx_destroy(c);
        return ZS_STREAM_ERROR;
    }
    *out = c;
    return ZS_OK;
}

void zs_ctx_destroy(zs_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    DevBuf *bufs[] = {&c->sd, &c->st, &c->work, &c->link, &c->mm, &c->maps, &c->chunk_far, &c->segmap, &c->supmap, &c->seg_entry, &c->seg_symbase, &c->seg_stale, &c->entry, &c->symbase, &c->stale, &c->syms,
                      &c->blk_end, &c->blk_top, &c->blocks, &c->trees, &c->info, &c->tile_bits, &c->pieces, &c->scratch, &c->stage_in, &c->stage_out, &c->wr, &c->inf_desc, &c->inf_state, &c->par_ps, &c->par_st, &c->par_work, &c->par_cbits, &c->par_ccnt, &c->par_surv, &c->par_scnt,
                      &c->par_cands, &c->par_tabs, &c->par_toktabs, &c->par_toks, &c->par_ctoks, &c->par_tokstat, &c->par_tails, &c->par_retry, &c->par_fxtab, &c->par_blocks, &c->par_cells, &c->par_windows, &c->par_fail, &c->run_syms, &c->run_bits,
                      &c->run_scratch, &c->run_outs, &c->run_fail, &c->adl_tr, &c->adl_res, &c->plan_blk, &c->ins_bits, &c->mm_bak, &c->cut_pos, &c->cut_bkt, &c->win_groups, &c->win_sg, &c->win_maps, &c->win_entries, &c->persist_bak, &c->resume_flag, &c->rle_tiles, &c->own_in, &c->fr_chunks, &c->fr_meta, &c->fr_planes, &c->fr_prov, &c->fr_base, &c->fr_counters, &c->spec_rec, &c->spec_flags, &c->spec_syms};
    for (DevBuf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (DevBuf &b : c->png)
        if (b.p) (void)hipFree(b.p);
    if (c->crc_tab) (void)hipFree(c->crc_tab);
    if (c->crc32_tab) (void)hipFree(c->crc32_tab);
    for (auto &e : c->ev_png)
        if (e) (void)hipEventDestroy(e);
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->plan_pin) (void)hipHostFree(c->plan_pin);
    delete c->plan;
    if (c->ev_verdict) (void)hipEventDestroy(c->ev_verdict);
    if (c->pin_io) (void)hipHostFree(c->pin_io);
    if (c->pin_out) (void)hipHostFree(c->pin_out);
    for (auto &e : c->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : c->ev_spec)
        if (e) (void)hipEventDestroy(e);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_pre0) (void)hipEventDestroy(c->ev_pre0);
    if (c->ev_pre) (void)hipEventDestroy(c->ev_pre);
    if (c->ev_syms) (void)hipEventDestroy(c->ev_syms);
    if (c->ev_part0) (void)hipEventDestroy(c->ev_part0);
    for (auto &e : c->ev_part1)
        if (e) (void)hipEventDestroy(e);
    if (c->aux) (void)hipStreamDestroy(c->aux);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *zs_ctx_last_error(const zs_ctx *c) { return c ? c->err.c_str() : "no context"; }

int64_t zs_deflate_bound(int64_t n) { return n + (n >> 3) + 1024; }

void zs_ctx_set_profiling(zs_ctx *c, int enable) {
    if (c) c->profiling = enable != 0;
}
int zs_ctx_stage_count(const zs_ctx *) { return kStCount; }
int64_t zs_ctx_counter(const zs_ctx *c, const char *name) {
    if (!c || !name) return -1;
    const std::string k(name);
    if (k == "fast_rounds") return c->fast_rounds;        // rounds of the last call's DeflateFast over its chunks (0: a workgroup per stream)
    if (k == "fast_fallbacks") return c->fast_fallbacks;  // speculative DeflateFast batches redone sequentially
    if (k == "round_runs") return c->round_runs;          // batches with streams in the batched cut rounds
    if (k == "cut_rounds") return c->cut_rounds;
    if (k == "lit_fallbacks") return c->lit_fallbacks;    // batches run again with a stream on the literal engine
    if (k == "lit_engine_bytes") return c->lit_engine_bytes;  // input bytes the one-wave literal engine has parsed (all calls)
    // the last deflate call's speculative chunk walk (levels 4-9): streams that tried it, those of them that took the maps
    // after all, chunks whose guessed entry was wrong
    if (k == "spec_streams") return c->spec_streams;
    if (k == "spec_fallbacks") return c->spec_fallbacks;
    if (k == "spec_periodic") return c->spec_periodic;  // ... fallbacks that were never walked (the match kernel's count of RUNS tiles)
    if (k == "spec_wrong_chunks") return c->spec_wrong_chunks;
    if (k == "plan_reused") return c->plan_reused;  // 1: the last deflate call took the plan of the call before (same shape)
    if (k == "inf_lane_streams") return c->inf_lane_streams;  // streams of the last inflate call with blocks for the lane decoder
    if (k == "inf_wave_streams") return c->inf_wave_streams;  // ... at or above the parallel minimum that run_inflate_par handed to `rest`
    if (k == "png_segments") return c->png_segments;  // segments the last zs_png_unfilter_batch_device call found
    return -1;
}

int64_t zs_ctx_debug_read(zs_ctx *c, const char *name, void *out, int64_t cap) {
    if (!c || !name || !out || !c->st.p) return -1;
    const std::string k(name);
    (void)hipSetDevice(c->device);
    StreamState ss;
    if (hipMemcpy(&ss, c->st.p, sizeof ss, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const void *src = nullptr;
    int64_t bytes = 0;
    const int32_t state[6] = {ss.tail_p, ss.tail_kind, (int32_t)ss.tail_pend, ss.k_done, ss.preins, (int32_t)ss.body_syms};
    if (k == "state") {
        if (cap < (int64_t)sizeof state) return -1;
        memcpy(out, state, sizeof state);
        return sizeof state;
    }
    if (k == "blk_end") src = dev<int32_t>(c->blk_end) + c->dbg_blk_off, bytes = 4 * (int64_t)(ss.body_syms / kBlockSyms);
    else if (k == "blk_top") src = dev<int32_t>(c->blk_top) + c->dbg_blk_off, bytes = 4 * (int64_t)(ss.body_syms / kBlockSyms);
    else if (k == "symbase") src = dev<uint32_t>(c->symbase) + c->dbg_chunk_off, bytes = 4 * c->dbg_nchunks;
    else if (k == "spec_base") src = dev<uint32_t>(c->spec_rec) + c->dbg_n_spec, bytes = 4 * c->dbg_spec_n;  // (the first stream's spec_off is 0)
    else return -1;
    if (bytes > cap || (bytes > 0 && !src)) return -1;
    if (bytes > 0 && hipMemcpy(out, src, (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return bytes;
}

const char *zs_ctx_stage_name(const zs_ctx *c, int s) {
    static const char *const inf_names[6] = {"inf_find", "inf_measure", "inf_chain", "inf_decode", "inf_windows", "inf_resolve"};
    if (s == kStCrc32 || s == kStSpecCompact || s == kStPngExpand || s == kStPngSplit || s == kStPngPack || s == kStPngSurvey || s == kStPngCompose || s == kStPngDiff || s == kStPngCrop || s == kStPart1 || s == kStChunk) return kStageNames[s];  // appended stages keep their names whatever the last call was: KC (the CRC-32 calls, the framing of PNG files, the check and gather of their chunks), KSc (the speculative walk's compaction), KX (the expansion to RGBA), KS (the Adam7 split), KG (the pack from RGBA), KV (the survey), KM (the frames of an animation composed), KD (the frame diff), the crop, the part-1 chain of a deflate call whose back end splits, and KN (the chunked-array kernels)
    if (c && c->last_op == 1) return s >= 0 && s < 6 ? inf_names[s] : "";
    // levels 1-3: DeflateFast for the lanes of a wave runs where the lazy parse has its expand stage, and the speculative
    // chunk runs (run / verify / stitch) are timed with the tail engine
    if (c && c->last_op == 2 && s == kStExpand) return "fast_sweep";
    if (c && c->last_op == 2 && s == kStTail) return "fast_runs+tail";
    return s >= 0 && s < kStCount ? kStageNames[s] : "";
}
double zs_ctx_stage_ms(const zs_ctx *c, int s) { return c && s >= 0 && s < kStCount ? c->stage_ms[s] : 0.0; }

int zs_deflate_batch_device(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out,
                            const int64_t *out_cap, int64_t *out_len, int *status, int level, int strategy, int hash_variant,
                            void *hip_stream) {
    if (!check_args(c, n, in_len, level, strategy)) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    // a batch whose workspace (~17 bytes per input byte) does not fit the device's free memory runs in sub-batches: the
    // streams are independent, the bytes the same
    int rc = ZS_OK;
    for (int lo = 0; lo < n;) {
        const int hi = batch_prefix_that_fits(c, n, in_len, out_cap, lo, 19);
        if (!run_pipeline(c, hi - lo, in + lo, in_len + lo, out + lo, out_cap + lo, out_len + lo, status ? status + lo : nullptr, level, strategy,
                          hash_variant, s) && rc == ZS_OK)
            rc = c->err == "buffer error" ? ZS_BUF_ERROR : ZS_STREAM_ERROR;
        lo = hi;
    }
    return rc;
}

int zs_deflate_writes_batch_device(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, const int64_t *const *write_ends,
                                   const int64_t *n_writes, void *const *out, const int64_t *out_cap, int64_t *out_len, int *status, int level,
                                   int strategy, int hash_variant, void *hip_stream) {
    if (!write_ends) return zs_deflate_batch_device(c, n, in, in_len, out, out_cap, out_len, status, level, strategy, hash_variant, hip_stream);
    if (!check_args(c, n, in_len, level, strategy)) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    // every list is checked before any device work: a malformed one anywhere fails the call (zs_core.h write_list_ends)
    std::vector<WriteSpec> specs((size_t)n);
    std::vector<const WriteSpec *> ptrs((size_t)n, nullptr);
    for (int i = 0; i < n; i++) {
        if (!write_ends[i] || (n_writes && n_writes[i] <= 0)) continue;  // one Write
        if (!n_writes || !write_list_ends(write_ends[i], n_writes[i], in_len[i], specs[(size_t)i].ends)) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        if (specs[(size_t)i].ends.empty()) continue;  // at most one distinct end
        specs[(size_t)i].flush.assign(specs[(size_t)i].ends.size(), 0);
        ptrs[(size_t)i] = &specs[(size_t)i];
    }
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    int rc = ZS_OK;
    for (int lo = 0; lo < n;) {  // sub-batches, as zs_deflate_batch_device
        const int hi = batch_prefix_that_fits(c, n, in_len, out_cap, lo, 19);
        if (!run_pipeline(c, hi - lo, in + lo, in_len + lo, out + lo, out_cap + lo, out_len + lo, status ? status + lo : nullptr, level, strategy,
                          hash_variant, s, ptrs.data() + lo) && rc == ZS_OK)
            rc = c->err == "buffer error" ? ZS_BUF_ERROR : ZS_STREAM_ERROR;
        lo = hi;
    }
    return rc;
}

int zs_deflate_writes_device(zs_ctx *c, const void *in, int64_t in_len, const int64_t *write_ends, int64_t n_writes, void *out,
                             int64_t out_cap, int64_t *out_len, int level, int strategy, int hash_variant, void *hip_stream) {
    if (!check_args(c, 1, &in_len, level, strategy)) return ZS_STREAM_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    WriteSpec ws;
    if (!write_list_ends(write_ends, n_writes, in_len, ws.ends)) {
        c->err = "stream error";
        return ZS_STREAM_ERROR;
    }
    ws.flush.assign(ws.ends.size(), 0);
    const WriteSpec *const one = &ws;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    int st = 0;
    if (!run_pipeline(c, 1, &in, &in_len, &out, &out_cap, out_len, &st, level, strategy, hash_variant, s, ws.ends.size() > 1 ? &one : nullptr))
        return c->err == "buffer error" ? ZS_BUF_ERROR : ZS_STREAM_ERROR;
    return ZS_OK;
}

namespace {
int deflate_batch_host_once(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out, const int64_t *out_cap,
                            int64_t *out_len, int *status, int level, int strategy, int hash_variant) {
    std::vector<const void *> din((size_t)n);
    std::vector<void *> dout((size_t)n);
    std::vector<int64_t> dcap((size_t)n);
    size_t tin = 0, tout = 0;
    for (int i = 0; i < n; i++) {
        tin += ((size_t)in_len[i] + 255) & ~(size_t)255;
        dcap[(size_t)i] = out_cap[i];
        tout += ((size_t)out_cap[i] + 255) & ~(size_t)255;
    }
    auto chk = [&](hipError_t e, const char *what) {
        if (e != hipSuccess) fail(c, what, e);
        return e == hipSuccess;
    };
    if (!ensure(c, c->stage_in, tin + 256) || !ensure(c, c->stage_out, tout + 256)) return ZS_MEM_ERROR;
    size_t oi = 0, oo = 0;
    for (int i = 0; i < n; i++) {
        din[(size_t)i] = (uint8_t *)c->stage_in.p + oi;
        dout[(size_t)i] = (uint8_t *)c->stage_out.p + oo;
        if (in_len[i] &&
            !chk(hipMemcpyAsync((void *)din[(size_t)i], in[i], (size_t)in_len[i], hipMemcpyHostToDevice, c->stream), "H2D"))
            return ZS_STREAM_ERROR;
        oi += ((size_t)in_len[i] + 255) & ~(size_t)255;
        oo += ((size_t)out_cap[i] + 255) & ~(size_t)255;
    }
    std::vector<int> st_local;
    if (!status) st_local.assign((size_t)n, 0), status = st_local.data();
    const bool ok = run_pipeline(c, n, din.data(), in_len, dout.data(), dcap.data(), out_len, status, level, strategy, hash_variant, c->stream);
    const std::string first_err = c->err;
    // streams that succeeded are delivered even when another stream of the batch failed (status[i] says which)
    for (int i = 0; i < n; i++)
        if (status[i] == 0 && out_len[i] > 0 && out_len[i] <= out_cap[i] &&
            !chk(hipMemcpyAsync(out[i], dout[(size_t)i], (size_t)out_len[i], hipMemcpyDeviceToHost, c->stream), "D2H"))
            return ZS_STREAM_ERROR;
    if (!chk(hipStreamSynchronize(c->stream), "sync")) return ZS_STREAM_ERROR;
    if (!ok) {
        c->err = first_err;
        return first_err == "buffer error" ? ZS_BUF_ERROR : ZS_STREAM_ERROR;
    }
    return ZS_OK;
}
}  // namespace

int zs_deflate_batch(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out, const int64_t *out_cap,
                     int64_t *out_len, int *status, int level, int strategy, int hash_variant) {
    if (!check_args(c, n, in_len, level, strategy)) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    // a batch that does not fit the device (staging for the inputs and outputs + ~17 bytes of workspace per input byte) runs
    // in sub-batches, one after the other through the same buffers: the streams are independent, the bytes the same
    int rc = ZS_OK;
    std::string first_err;
    for (int lo = 0; lo < n;) {
        const int hi = batch_prefix_that_fits(c, n, in_len, out_cap, lo, 20);
        const int r = deflate_batch_host_once(c, hi - lo, in + lo, in_len + lo, out + lo, out_cap + lo, out_len + lo, status ? status + lo : nullptr, level,
                                              strategy, hash_variant);
        if (r != ZS_OK && rc == ZS_OK) rc = r, first_err = c->err;
        lo = hi;
    }
    if (rc != ZS_OK) c->err = first_err;
    return rc;
}

int zs_adler32_device(zs_ctx *c, const void *d_buf, int64_t len, uint32_t seed, uint32_t *out, void *hip_stream) {
    if (!c || !out || len < 0 || len > 0x7FFFFFFF - 1024) return ZS_STREAM_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    uint32_t ad = 1;
    if (!device_adlers(c, 1, &d_buf, &len, nullptr, &ad, nullptr, s)) return ZS_STREAM_ERROR;
    *out = adler_combine(seed, ad, (uint64_t)len);
    return ZS_OK;
}

}  // extern "C"


// ------------------------------------------------------------------ inflate
namespace {
const char *const kInfMessages[kInfMsgCount] = {
    "", "unknown compression method", "invalid window size", "incorrect header check", "need dictionary", "invalid block type",
    "invalid stored block lengths", "too many length or distance symbols", "invalid bit length repeat",
    "oversubscribed dynamic bit lengths tree", "incomplete dynamic bit lengths tree", "oversubscribed literal/length tree",
    "incomplete literal/length tree", "oversubscribed distance tree", "incomplete distance tree", "empty distance tree with lengths",
    "invalid literal/length code", "invalid distance code", "buffer error", "buffer error", "incorrect data check"};
// the messages of a gzip member's own errors (zlib's, inflate.c), numbered on from the stream's
const char *const kGzipMessages[kInfMsgAll - kInfMsgCount] = {"unknown header flags set", "header crc mismatch", "incorrect length check"};
const char *inf_message(int m) { return m < kInfMsgCount ? kInfMessages[m] : kGzipMessages[m - kInfMsgCount]; }

// The container of an inflate call's streams (zs_inflate_wrap_batch_device).  body_off == nullptr: zlib streams.  Otherwise
// stream i's first block begins at byte body_off[i] and its last block ends it: no Adler-32 is read or computed.  in_used
// (may be null): the bytes of in[i] up to the stream's end, the Adler-32 included where there is one; 0 for a failing stream.
struct InfWrap {
    const int32_t *body_off = nullptr;
    int64_t *in_used = nullptr;
    int *msg = nullptr;  // (may be null) InfMsg of every failing stream, 0 for the others
};

bool run_inflate_seq(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out, const int64_t *out_cap,
                 int64_t *out_len, int *status, hipStream_t stream, uint32_t *adler_out = nullptr, int *msg_out = nullptr,
                 const InfWrap &wrap = InfWrap()) {
    const bool raw = wrap.body_off != nullptr;
    std::vector<InfDesc> d((size_t)n);
    for (int i = 0; i < n; i++) {
        d[(size_t)i] = {(const uint8_t *)in[i], (uint8_t *)out[i], in_len[i], out_cap[i]};
        if (raw) d[(size_t)i].body_off = wrap.body_off[i], d[(size_t)i].raw = 1;
    }
    if (!ensure(c, c->inf_desc, sizeof(InfDesc) * (size_t)n) || !ensure(c, c->inf_state, sizeof(InfState) * (size_t)n)) return false;
    std::vector<InfState> st((size_t)n);
    ZS_HIP(c, hipMemcpyAsync(c->inf_desc.p, d.data(), sizeof(InfDesc) * (size_t)n, hipMemcpyHostToDevice, stream));
    ZS_HIP(c, hipStreamSynchronize(stream));  // `d` is pageable host memory
    const bool prof = c->profiling;
    if (prof) (void)hipEventRecord(c->ev[0], stream);
    hipLaunchKernelGGL(zs_inflate_kernel, dim3((unsigned)n), dim3(64), kInfLds, stream, dev<InfDesc>(c->inf_desc),
                       dev<InfState>(c->inf_state));
    if (prof) (void)hipEventRecord(c->ev[1], stream);
    ZS_HIP(c, hipGetLastError());
    ZS_HIP(c, hipMemcpyAsync(st.data(), c->inf_state.p, sizeof(InfState) * (size_t)n, hipMemcpyDeviceToHost, stream));
    ZS_HIP(c, hipStreamSynchronize(stream));
    if (prof) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
        for (double &v : c->stage_ms) v = 0;
        c->stage_ms[0] = ms;  // reported under stage 0 for inflate calls
    }
    // Adler-32 of the produced bytes against the stored trailer, on the device, all finished streams in one pass
    // (Inflate.cs:300-345)
    std::vector<const void *> abuf;
    std::vector<int64_t> alen;
    std::vector<int> aidx;
    for (int i = 0; i < n; i++)
        if (st[(size_t)i].status == ZS_STREAM_END && !raw) abuf.push_back(out[i]), alen.push_back(st[(size_t)i].out_len), aidx.push_back(i);
    if (c->inf_probe == nullptr && n == 1) c->inf_used.assign(1, st[0].status == ZS_STREAM_END ? st[0].in_used : 0);
    std::vector<uint32_t> ads(abuf.size(), 1u);
    if (!device_adlers(c, (int)abuf.size(), abuf.data(), alen.data(), nullptr, ads.data(), nullptr, stream)) return false;
    for (size_t k = 0; k < aidx.size(); k++) {
        InfState &q = st[(size_t)aidx[k]];
        if (ads[k] != q.adler_stored) q.status = ZS_DATA_ERROR, q.msg = kInfBadCheck;
        else if (adler_out) adler_out[aidx[k]] = ads[k];
    }
    bool all_ok = true;
    for (int i = 0; i < n; i++) {
        out_len[i] = st[(size_t)i].out_len;
        const int code = st[(size_t)i].status;
        if (status) status[i] = code;
        if (msg_out) msg_out[i] = st[(size_t)i].msg;
        if (wrap.in_used) wrap.in_used[i] = code == ZS_STREAM_END ? st[(size_t)i].in_used : 0;
        if (code != ZS_STREAM_END) {
            if (all_ok) c->err = kInfMessages[st[(size_t)i].msg];
            all_ok = false;
        }
    }
    return all_ok;
}

// One piece of a stream that is decoded as it arrives (zs_inflate): the complete blocks in [start_bit, 8 in_len) of the
// device buffer `in`, behind `hist_have` bytes of history (device), into `out`.  status: ZS_OK -- stopped in front of a
// block that is not complete --, ZS_STREAM_END -- the trailer is behind it (its Adler-32 in *adler_stored; the caller
// keeps the running checksum) --, or the stream's error; good_bits: the bit behind the last complete block.
bool run_inflate_piece(zs_ctx *c, const void *in, int64_t in_len, bool first, int64_t start_bit, const void *hist, int hist_have, void *out, int64_t out_cap,
                       int64_t *out_len, int64_t *good_bits, int64_t *in_used, int *status, uint32_t *adler_stored, hipStream_t stream) {
    InfDesc d{(const uint8_t *)in, (uint8_t *)out, in_len, out_cap, (const uint8_t *)hist, first ? 0 : start_bit, hist_have, first ? 1 : 2};
    if (!ensure(c, c->inf_desc, sizeof(InfDesc)) || !ensure(c, c->inf_state, sizeof(InfState))) return false;
    InfState st;
    ZS_HIP(c, hipMemcpyAsync(c->inf_desc.p, &d, sizeof d, hipMemcpyHostToDevice, stream));
    ZS_HIP(c, hipStreamSynchronize(stream));
    hipLaunchKernelGGL(zs_inflate_kernel, dim3(1), dim3(64), kInfLds, stream, dev<InfDesc>(c->inf_desc), dev<InfState>(c->inf_state));
    ZS_HIP(c, hipGetLastError());
    ZS_HIP(c, hipMemcpyAsync(&st, c->inf_state.p, sizeof st, hipMemcpyDeviceToHost, stream));
    ZS_HIP(c, hipStreamSynchronize(stream));
    *out_len = st.out_len, *good_bits = st.good_bits, *in_used = st.in_used, *status = st.status, *adler_stored = st.adler_stored;
    if (st.status != ZS_OK && st.status != ZS_STREAM_END) c->err = kInfMessages[st.msg];
    return true;
}

// shorter streams go straight to the one-wave decoder (4 MB/s: 0.25 ms for a kilobyte of compressed text, what the block-parallel
// pass costs before it has decoded anything; until late in round 5 the line was drawn at 256 KiB -- a 600 KiB text stream took 120 ms,
// it takes 1.05 now, 256 streams of 64 KiB 1.25 instead of 14.2)
constexpr int64_t kParMinInput = 1024;

// Block-parallel path for the streams listed in `idx`; streams it cannot handle are appended to `rest`.
bool run_inflate_par(zs_ctx *c, const std::vector<int> &idx, const void *const *in, const int64_t *in_len, void *const *out,
                     const int64_t *out_cap, int64_t *out_len, int *status, hipStream_t stream, std::vector<int> &rest,
                     uint32_t *adler_out = nullptr, int *msg_out = nullptr, const InfWrap &wrap = InfWrap()) {
    const int m = (int)idx.size();
    const bool raw = wrap.body_off != nullptr;
    const int64_t trailer = raw ? 0 : 4;  // bytes of the stream behind its last block
    c->inf_lane_streams = 0;
    c->inf_wave_streams = 0;
    if (m == 0) return true;
    std::vector<ParStream> ps((size_t)m);
    int64_t nchunks = 0, ncand = 0, nblk = 0, ncells = 0, nfx = 0;
    std::vector<uint2> w_find;
    for (int j = 0; j < m; j++) {
        const int i = idx[(size_t)j];
        ParStream &p = ps[(size_t)j];
        p.in = (const uint8_t *)in[i], p.out = (uint8_t *)out[i], p.in_len = in_len[i], p.out_cap = out_cap[i];
        p.chunk_off = (int32_t)nchunks, p.nchunks = (int32_t)((in_len[i] + kFindChunk - 1) / kFindChunk);
        nchunks += p.nchunks;
        p.cand_off = (int32_t)ncand, p.max_cand = (int32_t)(in_len[i] / 128 + 64);
        ncand += p.max_cand;
        p.blk_off = (int32_t)nblk, p.max_blk = (int32_t)(in_len[i] / 96 + 64);
        nblk += p.max_blk;
        p.cell_off = ncells;
        p.fx_off = (int32_t)nfx, p.fx_regions = (int32_t)(in_len[i] * 8 / kFxRegionBits + 1);
        p.body_off = raw ? wrap.body_off[i] : 2, p.raw = raw ? 1 : 0;
        nfx += p.fx_regions;
        if (c->inf_probe) p.out_cap = (int64_t)0x7FFFFFFF - 1024;  // a probing call decodes nothing: any output size is fine
        else ncells += (out_cap[i] + 63) & ~63LL;
        for (int k = 0; k < p.nchunks; k++) w_find.push_back(make_uint2((unsigned)j, (unsigned)k));
    }
    if (!ensure(c, c->par_ps, sizeof(ParStream) * (size_t)m) || !ensure(c, c->par_st, sizeof(ParState) * (size_t)m) ||
        !ensure(c, c->par_work, sizeof(uint2) * (size_t)std::max<int64_t>(std::max<int64_t>(nchunks, ncand), nblk) + 64) ||
        !ensure(c, c->par_cbits, 8 * (size_t)nchunks * kFindMaxCand + 64) || !ensure(c, c->par_ccnt, 4 * (size_t)nchunks + 64) ||
        !ensure(c, c->par_surv, 4 * (size_t)nchunks * kFindMaxSurv + 64) || !ensure(c, c->par_scnt, 4 * (size_t)nchunks + 64) ||
        !ensure(c, c->par_cands, sizeof(ParCand) * (size_t)ncand) || !ensure(c, c->par_blocks, sizeof(ParBlock) * (size_t)nblk) ||
        !ensure(c, c->par_cells, 2 * (size_t)ncells + 64) || !ensure(c, c->par_fail, 4 * (size_t)m + 64))
        return false;
    std::vector<ParState> st((size_t)m);
    ZS_HIP(c, hipMemcpyAsync(c->par_ps.p, ps.data(), sizeof(ParStream) * (size_t)m, hipMemcpyHostToDevice, stream));
    ZS_HIP(c, hipMemcpyAsync(c->par_work.p, w_find.data(), sizeof(uint2) * w_find.size(), hipMemcpyHostToDevice, stream));
    ZS_HIP(c, hipMemsetAsync(c->par_fail.p, 0, 4 * (size_t)m + 64, stream));
    ZS_HIP(c, hipStreamSynchronize(stream));  // ps / w_find are pageable
    const ParStream *d_ps = dev<ParStream>(c->par_ps);
    ParState *d_st = dev<ParState>(c->par_st);
    const bool prof = c->profiling;
    auto mark = [&](int k) {
        if (prof) (void)hipEventRecord(c->ev[k], stream);
    };
    mark(0);
    hipLaunchKernelGGL(zs_inf_prefilter_kernel, dim3((unsigned)w_find.size()), dim3(256), 0, stream, d_ps, dev<uint2>(c->par_work),
                       dev<int32_t>(c->par_surv), dev<int32_t>(c->par_scnt));
    hipLaunchKernelGGL(zs_inf_check_kernel, dim3((unsigned)((w_find.size() + 1) / 2)), dim3(64), 0, stream, d_ps, dev<uint2>(c->par_work), (int)w_find.size(),
                       dev<int32_t>(c->par_surv), dev<int32_t>(c->par_scnt), dev<int64_t>(c->par_cbits), dev<int32_t>(c->par_ccnt));
    hipLaunchKernelGGL(zs_inf_flatten_kernel, dim3((unsigned)m), dim3(256), 0, stream, d_ps, d_st, dev<int64_t>(c->par_cbits),
                       dev<int32_t>(c->par_ccnt), dev<ParCand>(c->par_cands), m);
    // decode once (zs_inflate_tok.hip): the measuring pass writes tokens, the expand pass turns them into cells
    int64_t tok_total = 0;
    if (!ensure(c, c->par_tokstat, 128) || !ensure(c, c->par_tails, 4 * (size_t)kSbTailBuf * (size_t)m)) return false;
    hipLaunchKernelGGL(zs_inf_tails_kernel, dim3((unsigned)m), dim3(64), 0, stream, d_ps, dev<uint32_t>(c->par_tails));
    if (!c->inf_probe) {  // (a probing call decodes nothing: no slabs, the measuring pass stores no tokens)
        hipLaunchKernelGGL(zs_inf_tokalloc_kernel, dim3((unsigned)m), dim3(1024), 0, stream, d_ps, d_st, dev<ParCand>(c->par_cands));
        hipLaunchKernelGGL(zs_inf_tokbase_kernel, dim3(1), dim3(1024), 0, stream, d_st, m, dev<int64_t>(c->par_tokstat));
        ZS_HIP(c, hipMemcpyAsync(&tok_total, c->par_tokstat.p, 8, hipMemcpyDeviceToHost, stream));
    }
    mark(1);
    ZS_HIP(c, hipMemcpyAsync(st.data(), d_st, sizeof(ParState) * (size_t)m, hipMemcpyDeviceToHost, stream));
    ZS_HIP(c, hipStreamSynchronize(stream));
    std::vector<uint2> w;
    // (a stream whose candidate lists overflowed -- ok == 0: it goes to the sequential decoder -- is not measured: what
    // its list holds behind the overflow is whatever was in the buffer)
    for (int j = 0; j < m; j++)
        for (int k = 0; st[(size_t)j].ok && k < st[(size_t)j].ncand; k++) w.push_back(make_uint2((unsigned)j, (unsigned)k));
    if (getenv("ZS_DEBUG_INF")) {  // the finder's candidates per stream: count, range, order
        for (int j = 0; j < m; j++) {
            const int nc = st[(size_t)j].ncand;
            std::vector<ParCand> hc((size_t)std::max(nc, 1));
            if (nc) (void)hipMemcpy(hc.data(), dev<ParCand>(c->par_cands) + ps[(size_t)j].cand_off, sizeof(ParCand) * (size_t)nc, hipMemcpyDeviceToHost);
            int bad = 0;
            for (int k = 0; k < nc; k++) bad += hc[(size_t)k].bit < 16 || hc[(size_t)k].bit >= ps[(size_t)j].in_len * 8 || (k && hc[(size_t)k].bit <= hc[(size_t)k - 1].bit);
            fprintf(stderr, "[zs] inflate stream %d: %lld bytes, %d candidates (room for %d), ok %d, out of range or order: %d, first %lld last %lld\n", j,
                    (long long)ps[(size_t)j].in_len, nc, ps[(size_t)j].max_cand, st[(size_t)j].ok, bad, nc ? (long long)hc[0].bit : -1LL,
                    nc ? (long long)hc[(size_t)nc - 1].bit : -1LL);
        }
    }
    if (!w.empty()) {
        ZS_HIP(c, hipMemcpyAsync(c->par_work.p, w.data(), sizeof(uint2) * w.size(), hipMemcpyHostToDevice, stream));
        ZS_HIP(c, hipStreamSynchronize(stream));
        // one wave per candidate, its lanes on subsequences of the block (self-synchronising decode)
        if (!ensure(c, c->par_toktabs, sizeof(TokTabs) * w.size()) || !ensure(c, c->par_tabs, sizeof(LaneTabs) * w.size())) return false;
        // the tokens twice (the lanes' slabs, the blocks' lists); without room for them the blocks are decoded again lane by lane
        int mdbg = getenv("ZS_INF_MEASURE_DBG") ? atoi(getenv("ZS_INF_MEASURE_DBG")) : 0;
        // (behind the slabs: room for the blocks that are measured a second time, zs_inf_tokretry_kernel)
        const int64_t tok_reserve = c->inf_probe ? 0 : std::max<int64_t>(tok_total / 16, 2 << 20);
        if (!ensure(c, c->par_toks, 4 * (size_t)(tok_total + tok_reserve) + 64) || !ensure(c, c->par_ctoks, 4 * (size_t)(tok_total + tok_reserve) + 64)) {
            c->err.clear();
            if (!ensure(c, c->par_toks, 64) || !ensure(c, c->par_ctoks, 64)) return false;
            mdbg = 3;
        }
        int32_t *stats = nullptr;
        if (getenv("ZS_DEBUG_INF") && !c->inf_probe) {
            ZS_HIP(c, hipMemsetAsync((uint8_t *)c->par_tokstat.p + 16, 0, 64, stream));
            stats = (int32_t *)((uint8_t *)c->par_tokstat.p + 16);
        }
        hipLaunchKernelGGL(zs_inf_measure_tok_kernel, dim3((unsigned)w.size()), dim3(64), 0, stream, d_ps, d_st, dev<uint2>(c->par_work),
                           dev<ParCand>(c->par_cands), dev<TokTabs>(c->par_toktabs), dev<LaneTabs>(c->par_tabs), dev<uint32_t>(c->par_toks), dev<uint32_t>(c->par_ctoks), dev<uint32_t>(c->par_tails), stats, mdbg, nullptr, nullptr);
        if (mdbg != 3 && !c->inf_probe) {
            // blocks measured without room for their tokens: once more, with room for their known length
            if (!ensure(c, c->par_retry, 4 * (size_t)kTokRetryMax + 64)) return false;
            uint8_t *rb = (uint8_t *)c->par_retry.p;
            unsigned long long *d_cursor = (unsigned long long *)(rb + 4 * (size_t)kTokRetryMax);
            int32_t *d_rcnt = (int32_t *)(rb + 4 * (size_t)kTokRetryMax + 8);
            ZS_HIP(c, hipMemsetAsync(d_cursor, 0, 16, stream));
            hipLaunchKernelGGL(zs_inf_tokretry_kernel, dim3((unsigned)((w.size() + 255) / 256)), dim3(256), 0, stream, d_ps, dev<uint2>(c->par_work), (int)w.size(),
                               dev<ParCand>(c->par_cands), tok_total, tok_reserve, d_cursor, d_rcnt, (int32_t *)rb);
            hipLaunchKernelGGL(zs_inf_measure_tok_kernel, dim3((unsigned)std::min<size_t>(w.size(), (size_t)kTokRetryMax)), dim3(64), 0, stream, d_ps, d_st,
                               dev<uint2>(c->par_work), dev<ParCand>(c->par_cands), dev<TokTabs>(c->par_toktabs), dev<LaneTabs>(c->par_tabs), dev<uint32_t>(c->par_toks),
                               dev<uint32_t>(c->par_ctoks), dev<uint32_t>(c->par_tails), (int32_t *)nullptr, mdbg, d_rcnt, (int32_t *)rb);
        }
        if (stats) {
            int32_t hs[4] = {0, 0, 0, 0};
            ZS_HIP(c, hipMemcpyAsync(hs, stats, 16, hipMemcpyDeviceToHost, stream));
            ZS_HIP(c, hipStreamSynchronize(stream));
            fprintf(stderr, "[zs] inflate measure: %zu candidates, %d subsequences, %d re-entries met their first decode, %d decoded again in full, %d blocks without tokens; %lld tokens of room\n",
                    w.size(), hs[2], hs[1], hs[0], hs[3], (long long)tok_total);
        }
    }
    mark(2);
    // measured blocks carry tokens or, without room for those, checkpoints: the chain kernels hand them to the expand pass
    // or to the lane decoder (sub-blocks, one lane each); blocks that were not measured go to the wave decoder
    const bool measured = !w.empty();
    const bool chain_par = !getenv("ZS_INF_CHAIN_WALK");
    if (chain_par)
        hipLaunchKernelGGL(zs_inf_chain_par_kernel, dim3((unsigned)m), dim3(1024), kChainParLds, stream, d_ps, d_st, dev<ParCand>(c->par_cands),
                           dev<ParBlock>(c->par_blocks), measured ? 1 : 0);
    // a stream the finder's blocks do not chain (fixed-code or stored blocks among them): its fixed blocks found ahead of the walk,
    // a wave per 64 KiB (zs_inf_fixed_scan_kernel; the waves of the streams that chained leave at once)
    const FxEntry *d_fx = nullptr;
    static const bool fx_scan = !getenv("ZS_INF_NO_FIXED_SCAN");
    if (chain_par && fx_scan && !c->inf_probe && m <= 65535 && nfx > 0 && nfx < (1 << 22) &&
        ensure(c, c->par_fxtab, sizeof(FxEntry) * (size_t)nfx * kFxEntries + 64)) {
        int max_regions = 1;
        for (int j = 0; j < m; j++) max_regions = std::max(max_regions, (int)ps[(size_t)j].fx_regions);
        d_fx = dev<FxEntry>(c->par_fxtab);
        hipLaunchKernelGGL(zs_inf_fixed_scan_kernel, dim3((unsigned)max_regions, (unsigned)m), dim3(64), 0, stream, d_ps, d_st, dev<FxEntry>(c->par_fxtab));
    }
    hipLaunchKernelGGL(zs_inf_chain_kernel, dim3((unsigned)m), dim3(64), 0, stream, d_ps, d_st, dev<ParCand>(c->par_cands),
                       dev<ParBlock>(c->par_blocks), measured ? 1 : 0, (chain_par ? 1 : 0) | (c->inf_probe ? 2 : 0), d_fx);
    mark(3);
    ZS_HIP(c, hipMemcpyAsync(st.data(), d_st, sizeof(ParState) * (size_t)m, hipMemcpyDeviceToHost, stream));
    ZS_HIP(c, hipStreamSynchronize(stream));
    if (c->inf_probe) {
        // a probing call (zs_inflate: has the stream's end arrived?): the chain of blocks reached a final block and its
        // trailer lies inside the bytes -- or not yet; nothing is decoded
        const int64_t tb = (st[0].end_bit + 7) >> 3;
        *c->inf_probe = (m == 1 && st[0].ok && tb + 4 <= in_len[idx[0]]) ? tb + 4 : 0;
        return true;
    }
    w.clear();
    // windows are laid out by the block counts the chain found (not by the per-stream bounds the other tables use)
    int64_t total_blk = 0;
    for (int j = 0; j < m; j++)
        if (st[(size_t)j].ok) {
            for (int k = 0; k < st[(size_t)j].nblk; k++) w.push_back(make_uint2((unsigned)j, (unsigned)k));
            st[(size_t)j].win_off = (int32_t)total_blk;
            total_blk += st[(size_t)j].nblk;
        }
    std::vector<int32_t> bfail((size_t)m, 0);
    if (!w.empty()) {
        if (total_blk > 0x7FFFFFFF / 2 || !ensure(c, c->par_windows, (size_t)total_blk * kWSize + 64)) {
            // no room for the windows (streams cut into very many small blocks): the one-wave decoder needs none
            c->err.clear();
            for (int j = 0; j < m; j++) rest.push_back(idx[(size_t)j]);
            c->inf_wave_streams = m;
            return true;
        }
        // the window pass runs over groups of blocks (zs_inflate_par.hip, W): enough groups to give every CU one, none
        // shorter than a few blocks
        std::vector<WinGroup> groups;
        std::vector<int2> sgv((size_t)m, make_int2(0, 0));
        int n_ok = 0, n_slots = 0;
        for (int j = 0; j < m; j++) n_ok += st[(size_t)j].ok ? 1 : 0;
        for (int j = 0; j < m; j++) {
            if (!st[(size_t)j].ok) continue;
            const int nb = st[(size_t)j].nblk;
            int G = (256 + n_ok - 1) / n_ok;
            if (G > 16) G = 16;
            if (G > nb / 4) G = nb / 4;
            if (G < 1) G = 1;
            sgv[(size_t)j] = make_int2((int)groups.size(), G);
            for (int k = 0; k < G; k++) {
                const int first = (int)((int64_t)nb * k / G), last = (int)((int64_t)nb * (k + 1) / G);
                groups.push_back(WinGroup{j, first, last - first, k == 0 ? 0 : 1, k == 0 ? 0 : n_slots, 0});
                if (k) n_slots++;
            }
        }
        if (!ensure(c, c->win_groups, sizeof(WinGroup) * groups.size() + 64) || !ensure(c, c->win_sg, sizeof(int2) * (size_t)m + 64) ||
            !ensure(c, c->win_maps, 2 * (size_t)kWSize * (size_t)n_slots + 64) || !ensure(c, c->win_entries, (size_t)kWSize * (size_t)n_slots + 64))
            return false;
        ZS_HIP(c, hipMemcpyAsync(c->win_groups.p, groups.data(), sizeof(WinGroup) * groups.size(), hipMemcpyHostToDevice, stream));
        ZS_HIP(c, hipMemcpyAsync(c->win_sg.p, sgv.data(), sizeof(int2) * (size_t)m, hipMemcpyHostToDevice, stream));
        ZS_HIP(c, hipMemcpyAsync(d_st, st.data(), sizeof(ParState) * (size_t)m, hipMemcpyHostToDevice, stream));
        ZS_HIP(c, hipMemcpyAsync(c->par_work.p, w.data(), sizeof(uint2) * w.size(), hipMemcpyHostToDevice, stream));
        ZS_HIP(c, hipStreamSynchronize(stream));
        // (blocks with checkpoints and no tokens: the lane decoder and its flatten pass have work)
        for (int j = 0; j < m; j++) c->inf_lane_streams += st[(size_t)j].ok && st[(size_t)j].lane_blocks;
        const bool lane_work = c->inf_lane_streams > 0;
        if (measured)
            hipLaunchKernelGGL(zs_inf_expand_kernel, dim3((unsigned)w.size()), dim3(kExpThreads), kExpLds, stream, d_ps, d_st, dev<uint2>(c->par_work),
                               dev<ParBlock>(c->par_blocks), dev<TokTabs>(c->par_toktabs), dev<uint32_t>(c->par_ctoks), dev<uint16_t>(c->par_cells),
                               dev<int32_t>(c->par_fail), getenv("ZS_DEBUG_INF") ? (int32_t *)((uint8_t *)c->par_tokstat.p + 16) : nullptr);
        if (lane_work)
            hipLaunchKernelGGL(zs_inf_decode_lane_kernel, dim3((unsigned)((w.size() + kDecBlocks - 1) / kDecBlocks)), dim3(64), 0, stream, d_ps,
                               d_st, dev<uint2>(c->par_work), (int)w.size(), dev<ParBlock>(c->par_blocks), dev<LaneTabs>(c->par_tabs),
                               dev<uint16_t>(c->par_cells), dev<int32_t>(c->par_fail));
        hipLaunchKernelGGL(zs_inf_decode_kernel, dim3((unsigned)w.size()), dim3(64), 0, stream, d_ps, d_st, dev<uint2>(c->par_work),
                           dev<ParBlock>(c->par_blocks), dev<uint16_t>(c->par_cells), dev<int32_t>(c->par_fail));
        if (lane_work)
            hipLaunchKernelGGL(zs_inf_cellflat_kernel, dim3((unsigned)w.size()), dim3(256), 0, stream, d_ps, d_st, dev<uint2>(c->par_work),
                               dev<ParBlock>(c->par_blocks), dev<LaneTabs>(c->par_tabs), dev<uint16_t>(c->par_cells));
        mark(4);
        if (!groups.empty()) {
            hipLaunchKernelGGL(zs_inf_window_kernel, dim3((unsigned)groups.size()), dim3(1024), kWinMapLds, stream, d_ps, d_st, dev<WinGroup>(c->win_groups),
                               dev<ParBlock>(c->par_blocks), dev<uint16_t>(c->par_cells), dev<uint8_t>(c->par_windows), dev<uint16_t>(c->win_maps),
                               dev<uint8_t>(c->win_entries), 0);
            if (n_slots) {
                hipLaunchKernelGGL(zs_inf_winchain_kernel, dim3((unsigned)m), dim3(1024), 0, stream, d_st, dev<WinGroup>(c->win_groups), dev<int2>(c->win_sg),
                                   dev<uint8_t>(c->par_windows), dev<uint16_t>(c->win_maps), dev<uint8_t>(c->win_entries));
                hipLaunchKernelGGL(zs_inf_window_kernel, dim3((unsigned)groups.size()), dim3(1024), kWinMapLds, stream, d_ps, d_st,
                                   dev<WinGroup>(c->win_groups), dev<ParBlock>(c->par_blocks), dev<uint16_t>(c->par_cells), dev<uint8_t>(c->par_windows),
                                   dev<uint16_t>(c->win_maps), dev<uint8_t>(c->win_entries), 1);
            }
        }
        mark(5);
        hipLaunchKernelGGL(zs_inf_resolve_kernel, dim3((unsigned)w.size()), dim3(256), 0, stream, d_ps, d_st, dev<uint2>(c->par_work),
                           dev<ParBlock>(c->par_blocks), dev<uint16_t>(c->par_cells), dev<uint8_t>(c->par_windows));
        mark(6);
        ZS_HIP(c, hipGetLastError());
        ZS_HIP(c, hipMemcpyAsync(bfail.data(), c->par_fail.p, 4 * (size_t)m, hipMemcpyDeviceToHost, stream));
        ZS_HIP(c, hipStreamSynchronize(stream));
        if (getenv("ZS_DEBUG_INF")) {
            int32_t hs[16] = {};
            (void)hipMemcpy(hs, (uint8_t *)c->par_tokstat.p + 16, 64, hipMemcpyDeviceToHost);
            fprintf(stderr, "[zs] inflate expand: %d blocks with tokens, %d steps, %d rounds of pointer jumping; cycles / 256 of wave 0 in phases: scan %d, barrier %d, fetch+words %d, cells %d, rounds %d, out %d, barrier %d\n",
                    hs[6], hs[4], hs[5], hs[8], hs[9], hs[10], hs[11], hs[12], hs[13], hs[14]);
        }
        if (prof) {
            c->last_op = 1;
            for (double &v : c->stage_ms) v = 0;
            for (int k = 0; k < 6; k++) {
                float ms = 0;
                (void)hipEventElapsedTime(&ms, c->ev[k], c->ev[k + 1]);
                c->stage_ms[k] = ms;  // stages 0..5 of an inflate call: find, measure, chain, decode, windows, resolve
            }
        }
    }
    // Adler-32 trailer after the last block, byte aligned (Inflate.cs:300-345): all streams in one device pass
    std::vector<const void *> abuf, atr;
    std::vector<int64_t> alen;
    std::vector<int> aidx;
    for (int j = 0; j < m; j++) {
        const int i = idx[(size_t)j];
        const ParState &q = st[(size_t)j];
        const int64_t tb = (q.end_bit + 7) >> 3;
        if (!q.ok || bfail[(size_t)j] || tb + trailer > in_len[i]) {
            rest.push_back(i);  // not decodable here, or truncated: the sequential decoder classifies it
            c->inf_wave_streams++;
            continue;
        }
        abuf.push_back(out[i]), alen.push_back(q.out_len), atr.push_back((const uint8_t *)in[i] + tb), aidx.push_back(j);
    }
    std::vector<uint32_t> ads(abuf.size(), 1u);
    std::vector<int> aok(abuf.size(), raw ? 1 : 0);  // (a stream without an Adler-32 has none to compute or compare)
    if (!raw && !device_adlers(c, (int)abuf.size(), abuf.data(), alen.data(), atr.data(), ads.data(), aok.data(), stream)) return false;
    for (size_t k = 0; k < aidx.size(); k++) {
        const int j = aidx[k], i = idx[(size_t)j];
        out_len[i] = st[(size_t)j].out_len;
        status[i] = ZS_STREAM_END;
        if (m == 1) c->inf_used.assign(1, ((st[(size_t)j].end_bit + 7) >> 3) + 4);
        if (wrap.in_used) wrap.in_used[i] = aok[k] ? ((st[(size_t)j].end_bit + 7) >> 3) + trailer : 0;
        if (adler_out) adler_out[i] = ads[k];
        if (!aok[k]) {
            status[i] = ZS_DATA_ERROR;
            if (msg_out) msg_out[i] = kInfBadCheck;
            c->err = kInfMessages[kInfBadCheck];
        }
    }
    return true;
}

// One gzip member per in[i] (zs_wrap_host.inc): header kernel, raw inflate from the body's offset, KC, the trailers' compare.
bool inflate_gzip_members(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out, const int64_t *out_cap,
                          int64_t *out_len, int64_t *in_used, int *status, int *msg, hipStream_t stream);

bool run_inflate(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out, const int64_t *out_cap,
                 int64_t *out_len, int *status, hipStream_t stream, uint32_t *adler_out = nullptr, const InfWrap &wrap = InfWrap()) {
    std::vector<int> par, seq;
    static const int64_t par_min = getenv("ZS_INF_PAR_MIN") ? atoll(getenv("ZS_INF_PAR_MIN")) : kParMinInput;
    for (int i = 0; i < n; i++) (in_len[i] >= par_min ? par : seq).push_back(i);
    std::vector<int> st((size_t)n, 0), msg((size_t)n, -1);
    if (wrap.in_used) std::fill(wrap.in_used, wrap.in_used + n, (int64_t)0);
    if (!run_inflate_par(c, par, in, in_len, out, out_cap, out_len, st.data(), stream, seq, adler_out, msg.data(), wrap)) return false;
    bool ok = true;
    for (int i : par)
        if (std::find(seq.begin(), seq.end(), i) == seq.end() && st[(size_t)i] != ZS_STREAM_END) ok = false;
    if (!seq.empty()) {
        const int m = (int)seq.size();
        std::vector<const void *> sin((size_t)m);
        std::vector<void *> sout((size_t)m);
        std::vector<int64_t> slen((size_t)m), scap((size_t)m), solen((size_t)m);
        std::vector<int> sst((size_t)m), smsg((size_t)m, -1);
        std::vector<uint32_t> sad((size_t)m, 1u);
        for (int j = 0; j < m; j++) sin[(size_t)j] = in[seq[(size_t)j]], sout[(size_t)j] = out[seq[(size_t)j]], slen[(size_t)j] = in_len[seq[(size_t)j]], scap[(size_t)j] = out_cap[seq[(size_t)j]];
        // (the container goes along in the one-wave decoder's order)
        std::vector<int32_t> sbody;
        std::vector<int64_t> sused((size_t)m, 0);
        InfWrap swrap;
        if (wrap.body_off) {
            for (int j = 0; j < m; j++) sbody.push_back(wrap.body_off[seq[(size_t)j]]);
            swrap.body_off = sbody.data();
        }
        if (wrap.in_used) swrap.in_used = sused.data();
        if (!run_inflate_seq(c, m, sin.data(), slen.data(), sout.data(), scap.data(), solen.data(), sst.data(), stream, sad.data(), smsg.data(), swrap)) ok = false;
        for (int j = 0; j < m; j++) {
            if (wrap.in_used) wrap.in_used[seq[(size_t)j]] = sused[(size_t)j];
            out_len[seq[(size_t)j]] = solen[(size_t)j], st[(size_t)seq[(size_t)j]] = sst[(size_t)j], msg[(size_t)seq[(size_t)j]] = smsg[(size_t)j];
            if (adler_out) adler_out[seq[(size_t)j]] = sad[(size_t)j];
        }
    }
    // the call's message is that of its first failing stream in the caller's order, as its code is: the block-parallel pass and
    // the one-wave decoder each leave the message of the first stream that failed with them, and either may come first
    for (int i = 0; i < n; i++)
        if (st[(size_t)i] != ZS_STREAM_END) {
            if (msg[(size_t)i] > 0) c->err = kInfMessages[msg[(size_t)i]];
            break;
        }
    if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
    if (wrap.msg)
        for (int i = 0; i < n; i++) wrap.msg[i] = st[(size_t)i] != ZS_STREAM_END && msg[(size_t)i] > 0 ? msg[(size_t)i] : 0;
    return ok;
}
}  // namespace

extern "C" {

int zs_inflate_wrap_batch_device(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out,
                                 const int64_t *out_cap, int64_t *out_len, int64_t *in_used, int *status, int wrap, void *hip_stream) {
    if (!c || n < 0 || wrap < ZS_WRAP_ZLIB || wrap > ZS_WRAP_GZIP) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    // what the caller sees if anything fails before the results are known (as run_pipeline does for deflate)
    for (int i = 0; i < n; i++) {
        out_len[i] = 0;
        if (in_used) in_used[i] = 0;
        if (status) status[i] = ZS_STREAM_ERROR;
    }
    for (int i = 0; i < n; i++)
        if (in_len[i] < 0 || in_len[i] > 0x7FFFFFFF - 1024 || out_cap[i] < 0 || out_cap[i] > 0x7FFFFFFF - 1024) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    std::vector<int> st((size_t)n, ZS_STREAM_ERROR);
    InfWrap wr;
    wr.in_used = in_used;
    std::vector<int32_t> body;
    bool ok;
    if (wrap == ZS_WRAP_GZIP) {
        ok = inflate_gzip_members(c, n, in, in_len, out, out_cap, out_len, in_used, st.data(), nullptr, s);
    } else {
        if (wrap == ZS_WRAP_RAW) body.assign((size_t)n, 0), wr.body_off = body.data();
        ok = run_inflate(c, n, in, in_len, out, out_cap, out_len, st.data(), s, nullptr, wr);
    }
    if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
    if (ok) return ZS_OK;
    for (int v : st)
        if (v != ZS_STREAM_END) return v == ZS_OK ? ZS_STREAM_ERROR : v;
    return ZS_STREAM_ERROR;
}

int zs_inflate_batch_device(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out,
                            const int64_t *out_cap, int64_t *out_len, int *status, void *hip_stream) {
    return zs_inflate_wrap_batch_device(c, n, in, in_len, out, out_cap, out_len, nullptr, status, ZS_WRAP_ZLIB, hip_stream);
}

int zs_inflate_batch(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out, const int64_t *out_cap,
                     int64_t *out_len, int *status) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    size_t tin = 0, tout = 0;
    for (int i = 0; i < n; i++) {
        out_len[i] = 0;
        if (status) status[i] = ZS_STREAM_ERROR;
    }
    for (int i = 0; i < n; i++) {
        if (in_len[i] < 0 || in_len[i] > 0x7FFFFFFF - 1024 || out_cap[i] < 0 || out_cap[i] > 0x7FFFFFFF - 1024) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        tin += ((size_t)in_len[i] + 255) & ~(size_t)255, tout += ((size_t)out_cap[i] + 255) & ~(size_t)255;
    }
    if (!ensure(c, c->stage_in, tin + 256) || !ensure(c, c->stage_out, tout + 256)) return ZS_MEM_ERROR;
    std::vector<const void *> din((size_t)n);
    std::vector<void *> dout((size_t)n);
    size_t oi = 0, oo = 0;
    for (int i = 0; i < n; i++) {
        din[(size_t)i] = (uint8_t *)c->stage_in.p + oi;
        dout[(size_t)i] = (uint8_t *)c->stage_out.p + oo;
        if (in_len[i] && hipMemcpyAsync((void *)din[(size_t)i], in[i], (size_t)in_len[i], hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return ZS_STREAM_ERROR;
        oi += ((size_t)in_len[i] + 255) & ~(size_t)255;
        oo += ((size_t)out_cap[i] + 255) & ~(size_t)255;
    }
    std::vector<int> st((size_t)n, ZS_STREAM_ERROR);
    int rc = zs_inflate_batch_device(c, n, din.data(), in_len, dout.data(), out_cap, out_len, st.data(), c->stream);
    if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
    // only what a stream that ended cleanly produced goes back, and never more than the caller's buffer holds
    for (int i = 0; i < n; i++)
        if (st[(size_t)i] == ZS_STREAM_END && out_len[i] > 0 && out_len[i] <= out_cap[i] &&
            hipMemcpyAsync(out[i], dout[(size_t)i], (size_t)out_len[i], hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            return ZS_STREAM_ERROR;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return ZS_STREAM_ERROR;
    return rc;
}

}  // extern "C"

#include "zs_png_host.inc"
#include "zs_parts_host.inc"
#include "zs_wrap_host.inc"
#include "zs_zip_host.inc"
#include "zs_tiff_host.inc"
#include "zs_exr_host.inc"
#include "zs_chunk_host.inc"

// ------------------------------------------------------------------ multi-GPU batch entry points
// BASELINE north_star: "independent input buffers shard embarrassingly across the 8 GPUs of one node (no RCCL needed)".
// The unit of sharding is the buffer (a zlib stream cannot be split bit-exactly: 32 KiB history, sequential parse,
// bit-contiguous blocks).  Longest-processing-time partition by size, one host thread and one context per device, results
// in input order; no collective, no peer traffic.
extern "C" {

int zs_device_count(void) {
    int count = 0;
    return hipGetDeviceCount(&count) == hipSuccess ? count : 0;
}

int zs_partition(const int64_t *sizes, int n, int n_parts, int *part_of) {
    if (!sizes || !part_of || n < 0 || n_parts <= 0) return ZS_STREAM_ERROR;
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sizes[a] > sizes[b]; });  // ties keep input order
    std::vector<int64_t> load((size_t)n_parts, 0);
    for (int i : order) {
        int best = 0;
        for (int k = 1; k < n_parts; k++)
            if (load[(size_t)k] < load[(size_t)best]) best = k;  // ties go to the lowest part
        part_of[i] = best;
        load[(size_t)best] += sizes[i];
    }
    return ZS_OK;
}

}  // extern "C"

namespace {
template <class Fn>  // Fn(ctx, count, in, in_len, out, out_cap, out_len, status) -> code
int run_multi(zs_ctx *const *ctxs, int n_ctx, int n, const void *const *in, const int64_t *in_len, void *const *out,
              const int64_t *out_cap, int64_t *out_len, int *status, const int64_t *weights, const int *part_of, Fn fn) {
    if (!ctxs || n_ctx <= 0 || n < 0) return ZS_STREAM_ERROR;
    for (int k = 0; k < n_ctx; k++)
        if (!ctxs[k]) return ZS_STREAM_ERROR;
    // a context is one workspace and one pair of HIP streams: two host threads in it at once would corrupt both shares
    for (int k = 0; k < n_ctx; k++)
        for (int j = 0; j < k; j++)
            if (ctxs[j] == ctxs[k]) {
                ctxs[k]->err = "stream error: the same context passed twice";
                return ZS_STREAM_ERROR;
            }
    if (n == 0) return ZS_OK;
    std::vector<int> part((size_t)n);
    if (part_of) {
        for (int i = 0; i < n; i++) {
            if (part_of[i] < 0 || part_of[i] >= n_ctx) return ZS_STREAM_ERROR;
            part[(size_t)i] = part_of[i];
        }
    } else if (zs_partition(weights, n, n_ctx, part.data()) != ZS_OK) return ZS_STREAM_ERROR;
    std::vector<std::vector<int>> idx((size_t)n_ctx);
    for (int i = 0; i < n; i++) idx[(size_t)part[(size_t)i]].push_back(i);
    std::vector<int> rc((size_t)n_ctx, ZS_OK);
    std::vector<std::thread> th;
    for (int k = 0; k < n_ctx; k++) {
        if (idx[(size_t)k].empty()) continue;
        th.emplace_back([&, k]() {
            const std::vector<int> &ix = idx[(size_t)k];
            const size_t m = ix.size();
            std::vector<const void *> sin(m);
            std::vector<void *> sout(m);
            std::vector<int64_t> slen(m), scap(m), solen(m, 0);
            std::vector<int> sst(m, ZS_STREAM_ERROR);
            for (size_t j = 0; j < m; j++) sin[j] = in[ix[j]], sout[j] = out[ix[j]], slen[j] = in_len[ix[j]], scap[j] = out_cap[ix[j]];
            rc[(size_t)k] = fn(ctxs[k], (int)m, sin.data(), slen.data(), sout.data(), scap.data(), solen.data(), sst.data());
            for (size_t j = 0; j < m; j++) {
                out_len[ix[j]] = solen[j];
                if (status) status[ix[j]] = sst[j];
            }
        });
    }
    for (std::thread &t : th) t.join();
    for (int k = 0; k < n_ctx; k++)
        if (rc[(size_t)k] != ZS_OK) return rc[(size_t)k];
    return ZS_OK;
}
}  // namespace

extern "C" {

int zs_deflate_batch_multi(zs_ctx *const *ctxs, int n_ctx, int n, const void *const *in, const int64_t *in_len, void *const *out,
                           const int64_t *out_cap, int64_t *out_len, int *status, int level, int strategy, int hash_variant) {
    return run_multi(ctxs, n_ctx, n, in, in_len, out, out_cap, out_len, status, in_len, nullptr,
                     [=](zs_ctx *c, int m, const void *const *i, const int64_t *il, void *const *o, const int64_t *oc, int64_t *ol, int *st) {
                         return zs_deflate_batch(c, m, i, il, o, oc, ol, st, level, strategy, hash_variant);
                     });
}

int zs_deflate_batch_multi_device(zs_ctx *const *ctxs, int n_ctx, int n, const void *const *in, const int64_t *in_len, void *const *out,
                                  const int64_t *out_cap, int64_t *out_len, int *status, const int *part_of, int level, int strategy,
                                  int hash_variant) {
    if (!part_of) return ZS_STREAM_ERROR;
    return run_multi(ctxs, n_ctx, n, in, in_len, out, out_cap, out_len, status, in_len, part_of,
                     [=](zs_ctx *c, int m, const void *const *i, const int64_t *il, void *const *o, const int64_t *oc, int64_t *ol, int *st) {
                         return zs_deflate_batch_device(c, m, i, il, o, oc, ol, st, level, strategy, hash_variant, nullptr);
                     });
}

int zs_inflate_batch_multi(zs_ctx *const *ctxs, int n_ctx, int n, const void *const *in, const int64_t *in_len, void *const *out,
                           const int64_t *out_cap, int64_t *out_len, int *status) {
    // balanced by output capacity: the decoded size is what an inflate costs
    return run_multi(ctxs, n_ctx, n, in, in_len, out, out_cap, out_len, status, out_cap, nullptr,
                     [](zs_ctx *c, int m, const void *const *i, const int64_t *il, void *const *o, const int64_t *oc, int64_t *ol, int *st) {
                         return zs_inflate_batch(c, m, i, il, o, oc, ol, st);
                     });
}

// ... and over device pointers: every stream and its output already resident on the GPU of the context `part_of` names (the
// caller partitions with zs_partition -- by the decoded sizes -- and places them), so the data path of N GPUs has no PCIe in it
int zs_inflate_batch_multi_device(zs_ctx *const *ctxs, int n_ctx, int n, const void *const *in, const int64_t *in_len, void *const *out,
                                  const int64_t *out_cap, int64_t *out_len, int *status, const int *part_of) {
    if (!part_of) return ZS_STREAM_ERROR;
    return run_multi(ctxs, n_ctx, n, in, in_len, out, out_cap, out_len, status, out_cap, part_of,
                     [](zs_ctx *c, int m, const void *const *i, const int64_t *il, void *const *o, const int64_t *oc, int64_t *ol, int *st) {
                         return zs_inflate_batch_device(c, m, i, il, o, oc, ol, st, nullptr);
                     });
}

}  // extern "C"

#include "zs_stream_api.inc"
