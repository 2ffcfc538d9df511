// zs_plan_key.h -- the shape of a deflate call: everything the planner (zs_plan.h plan_streams) reads.  Two calls whose keys are
// equal get the same plan -- descriptors but for the caller's pointers, work lists, geometry, workspace sizes -- so the second
// takes the first's ("A same-shaped call takes the plan of the one before").  The planner has no other way
// to the environment than the PlanEnv in here: what it reads is in the key because there is nowhere else to read it from
// (tests/cpp/test_plan.cpp compiles it with getenv poisoned).  No HIP in here: tests/cpp/test_plan_key.cpp walks the fields on
// the host.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace zs {

// The environment switches of the planning, as given: PlanEnv is the one reader of these names -- once per call, in
// plan_env_read -- and the planner and the launches take them from it (the values the engine makes of them: zs_plan.h
// plan_spec_bits and its neighbours).  A plan made under one setting does not serve a call under another.
// no_live_list is not the planning's but decides what a call leaves where the plan lives: with 64 streams or more a call
// rewrites the block list of the work array from its own block counts (zs_live_fill_kernel) unless ZS_NO_LIVE_LIST is set, and
// a call that has the switch set reads the list as zs_worklist_kernel made it -- so it must not take the plan of one that had not.
// spec_warm is not the planning's either: the walk's kernels get it as an argument and no size depends on it.  It stays in the
// key with its neighbours ZS_SPEC_LEN and ZS_SPEC_MIN, which are: a measurement that changes one of the three plans afresh.
struct PlanEnv {
    bool no_rle_multi = false, no_fast_vec = false, fast_no_rounds = false, no_spec = false, no_fast_multi = false, no_fast_resume = false,
         no_rle_runs = false, no_resume_rounds = false, no_live_list = false;
    bool has_fr_ratio = false, has_fr_chunk = false, has_fast_chunk = false, has_spec_len = false, has_spec_warm = false, has_spec_min = false,
         has_fast_min_input = false;
    int spec_len = 0, spec_warm = 0, fast_chunk = 0;  // (each as atoi / atoll / atof gives it; 0 where its has_ flag is not set)
    int64_t spec_min = 0, fr_chunk = 0, fast_min_input = 0;
    double fr_ratio = 0;
};
inline PlanEnv plan_env_read() {
    PlanEnv e;
    e.no_rle_multi = getenv("ZS_NO_RLE_MULTI") != nullptr, e.no_fast_vec = getenv("ZS_NO_FAST_VEC") != nullptr;
    e.fast_no_rounds = getenv("ZS_FAST_NO_ROUNDS") != nullptr, e.no_spec = getenv("ZS_NO_SPEC") != nullptr;
    e.no_fast_multi = getenv("ZS_NO_FAST_MULTI") != nullptr, e.no_fast_resume = getenv("ZS_NO_FAST_RESUME") != nullptr;
    e.no_rle_runs = getenv("ZS_NO_RLE_RUNS") != nullptr, e.no_resume_rounds = getenv("ZS_NO_RESUME_ROUNDS") != nullptr;
    e.no_live_list = getenv("ZS_NO_LIVE_LIST") != nullptr;
    if (const char *v = getenv("ZS_SPEC_LEN")) e.has_spec_len = true, e.spec_len = atoi(v);
    if (const char *v = getenv("ZS_SPEC_WARM")) e.has_spec_warm = true, e.spec_warm = atoi(v);
    if (const char *v = getenv("ZS_SPEC_MIN")) e.has_spec_min = true, e.spec_min = atoll(v);
    if (const char *v = getenv("ZS_FAST_CHUNK")) e.has_fast_chunk = true, e.fast_chunk = atoi(v);
    if (const char *v = getenv("ZS_FR_CHUNK")) e.has_fr_chunk = true, e.fr_chunk = atoll(v);
    if (const char *v = getenv("ZS_FR_RATIO")) e.has_fr_ratio = true, e.fr_ratio = atof(v);
    static const char *const fast_min = getenv("ZS_FAST_MIN_INPUT");  // (read once per process)
    if (fast_min) e.has_fast_min_input = true, e.fast_min_input = atoll(fast_min);
    return e;
}
inline bool plan_env_equal(const PlanEnv &a, const PlanEnv &b) {
    return a.no_rle_multi == b.no_rle_multi && a.no_fast_vec == b.no_fast_vec && a.fast_no_rounds == b.fast_no_rounds && a.no_spec == b.no_spec &&
           a.no_fast_multi == b.no_fast_multi && a.no_fast_resume == b.no_fast_resume && a.no_rle_runs == b.no_rle_runs &&
           a.no_resume_rounds == b.no_resume_rounds && a.no_live_list == b.no_live_list && a.has_fr_ratio == b.has_fr_ratio && a.has_fr_chunk == b.has_fr_chunk &&
           a.has_fast_chunk == b.has_fast_chunk && a.has_spec_len == b.has_spec_len && a.has_spec_warm == b.has_spec_warm && a.has_spec_min == b.has_spec_min &&
           a.has_fast_min_input == b.has_fast_min_input && a.spec_len == b.spec_len && a.spec_warm == b.spec_warm && a.fast_chunk == b.fast_chunk &&
           a.spec_min == b.spec_min && a.fr_chunk == b.fr_chunk && a.fast_min_input == b.fast_min_input && a.fr_ratio == b.fr_ratio;
}

// The Writes of one stream (ZlibOutputStream.WriteCore): cumulative ends, the FlushMode of each, the caller's output
// chunk size and whether the stream is raw deflate.
struct WriteSpec {
    std::vector<int64_t> ends;
    std::vector<uint8_t> flush;
    int chunk = 512;
    bool raw = false;
    bool flushing() const {
        for (uint8_t f : flush)
            if (f) return true;
        return false;
    }
};

// One stream's Writes as the key keeps them; present == false: the stream is one Write.
struct PlanKeyWrites {
    bool present = false, raw = false;
    int chunk = 512;
    std::vector<int64_t> ends;
    std::vector<uint8_t> flush;
};
inline bool plan_writes_equal(const PlanKeyWrites &a, const PlanKeyWrites &b) {
    return a.present == b.present && a.raw == b.raw && a.chunk == b.chunk && a.ends == b.ends && a.flush == b.flush;
}

struct PlanKey {
    int n = 0, level = 0, strategy = 0, hash_variant = 0;
    int force_seq = 0;  // the call is a batch run again (1: the sweeps, 2: one run per stream)
    // paths whose plan depends on more than the arguments (an incremental run's state, the re-entry behind the cut rounds, streams
    // forced to the literal engine, a call that may not take the rounds): a key with any of them set equals no key, itself included
    bool incremental = false, rounds = false, forced_lit = false, no_rounds = false;
    std::vector<int64_t> in_len, out_cap;
    std::vector<PlanKeyWrites> writes;  // empty: no stream of the call has a Write list
    PlanEnv env;
};
inline bool plan_key_reusable(const PlanKey &k) { return !k.incremental && !k.rounds && !k.forced_lit && !k.no_rounds && k.force_seq == 0; }
inline bool plan_key_equal(const PlanKey &a, const PlanKey &b) {
    if (!plan_key_reusable(a) || !plan_key_reusable(b)) return false;
    if (a.n != b.n || a.level != b.level || a.strategy != b.strategy || a.hash_variant != b.hash_variant || a.force_seq != b.force_seq) return false;
    if (a.in_len != b.in_len || a.out_cap != b.out_cap || a.writes.size() != b.writes.size()) return false;
    for (size_t i = 0; i < a.writes.size(); i++)
        if (!plan_writes_equal(a.writes[i], b.writes[i])) return false;
    return plan_env_equal(a.env, b.env);
}

// The key of a call, into `k` (its vectors keep their room from call to call).  `writes`: null, or one entry per stream, each null
// or that stream's Writes.
inline void plan_key_fill(PlanKey &k, int n, const int64_t *in_len, const int64_t *out_cap, int level, int strategy, int hash_variant, int force_seq,
                          bool incremental, bool rounds, bool forced_lit, bool no_rounds, const WriteSpec *const *writes, const PlanEnv &env) {
    k.n = n, k.level = level, k.strategy = strategy, k.hash_variant = hash_variant, k.force_seq = force_seq;
    k.incremental = incremental, k.rounds = rounds, k.forced_lit = forced_lit, k.no_rounds = no_rounds;
    k.in_len.assign(in_len, in_len + n);
    k.out_cap.assign(out_cap, out_cap + n);
    bool any = false;
    for (int i = 0; i < n && writes; i++) any = any || writes[i] != nullptr;
    k.writes.resize(any ? (size_t)n : 0);
    for (size_t i = 0; i < k.writes.size(); i++) {
        PlanKeyWrites &w = k.writes[i];
        const WriteSpec *v = writes[i];
        w.present = v != nullptr;
        w.raw = v && v->raw, w.chunk = v ? v->chunk : 512;
        if (v) w.ends = v->ends, w.flush = v->flush;
        else w.ends.clear(), w.flush.clear();
    }
    k.env = env;
}

}  // namespace zs
