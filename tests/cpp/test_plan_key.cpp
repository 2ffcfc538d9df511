// The shape key of a deflate call (zlibstream_amd/csrc/zs_plan_key.h) on the host: two keys built from the same arguments are
// equal; a change to any single field makes them unequal; a key of a path that is never reused equals nothing, itself included.
// Stand-alone: g++ -fsanitize=address,undefined tests/cpp/test_plan_key.cpp && ./a.out
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_plan_key.h"

using namespace zs;

namespace {
int failures = 0, checks = 0;
void expect(bool ok, const std::string &what) {
    checks++;
    if (!ok) failures++, printf("FAIL: %s\n", what.c_str());
}

// the arguments of a call, as run_pipeline has them
struct Args {
    int n = 3, level = 6, strategy = 0, hash_variant = 0, force_seq = 0;
    bool incremental = false, rounds = false, forced_lit = false, no_rounds = false;
    std::vector<int64_t> in_len{70000, 65536, 1}, out_cap{80000, 75000, 64};
    bool with_writes = true;
    std::vector<int64_t> ends0{100, 30000, 70000}, ends2{1};
    std::vector<uint8_t> flush0{0, 0, 0}, flush2{0};
    int chunk0 = 512, chunk2 = 512;
    bool raw0 = false, raw2 = false;
    bool stream1_has_writes = false;
    std::vector<int64_t> ends1{65536};
    std::vector<uint8_t> flush1{0};
    PlanEnv env;
};
PlanKey key_of(const Args &a) {
    WriteSpec v0, v1, v2;
    v0.ends = a.ends0, v0.flush = a.flush0, v0.chunk = a.chunk0, v0.raw = a.raw0;
    v1.ends = a.ends1, v1.flush = a.flush1;
    v2.ends = a.ends2, v2.flush = a.flush2, v2.chunk = a.chunk2, v2.raw = a.raw2;
    const WriteSpec *ptrs[3] = {&v0, a.stream1_has_writes ? &v1 : nullptr, &v2};
    PlanKey k;
    plan_key_fill(k, a.n, a.in_len.data(), a.out_cap.data(), a.level, a.strategy, a.hash_variant, a.force_seq, a.incremental, a.rounds, a.forced_lit, a.no_rounds,
                  a.with_writes ? ptrs : nullptr, a.env);
    return k;
}
}  // namespace

int main() {
    const Args base;
    expect(plan_key_equal(key_of(base), key_of(base)), "two keys from the same arguments are equal");
    {
        // the key is a copy: it does not look at the caller's arrays after it was made
        Args a = base;
        const PlanKey k = key_of(a);
        a.in_len[0]++, a.ends0[1]++;
        expect(plan_key_equal(k, key_of(base)), "a key keeps its own copy of lengths and Write ends");
    }
    {
        // a key filled twice (the vectors keep their room): the second fill leaves nothing of the first
        PlanKey k = key_of(base);
        Args a = base;
        a.with_writes = false;
        plan_key_fill(k, a.n, a.in_len.data(), a.out_cap.data(), a.level, a.strategy, a.hash_variant, 0, false, false, false, false, nullptr, a.env);
        expect(plan_key_equal(k, key_of(a)) && !plan_key_equal(k, key_of(base)), "a refilled key is the key of the second call");
    }
    // every single field: the change, by name
    const std::vector<std::pair<const char *, std::function<void(Args &)>>> changes = {
        {"n", [](Args &a) { a.n = 2, a.with_writes = false; }},
        {"level", [](Args &a) { a.level = 5; }},
        {"strategy", [](Args &a) { a.strategy = 1; }},
        {"hash_variant", [](Args &a) { a.hash_variant = 1; }},
        {"in_len[0]", [](Args &a) { a.in_len[0]++; }},
        {"in_len[1]", [](Args &a) { a.in_len[1]--; }},
        {"in_len[2]", [](Args &a) { a.in_len[2]++; }},
        {"out_cap[0]", [](Args &a) { a.out_cap[0]++; }},
        {"out_cap[2]", [](Args &a) { a.out_cap[2]--; }},
        {"no Write lists at all", [](Args &a) { a.with_writes = false; }},
        {"a Write list for stream 1", [](Args &a) { a.stream1_has_writes = true; }},
        {"a Write end", [](Args &a) { a.ends0[1]++; }},
        {"one Write more", [](Args &a) { a.ends0.insert(a.ends0.begin(), 50), a.flush0.push_back(0); }},
        {"one Write fewer", [](Args &a) { a.ends0.erase(a.ends0.begin()), a.flush0.pop_back(); }},
        {"a flush mode", [](Args &a) { a.flush0[1] = 2; }},
        {"the last stream's flush mode", [](Args &a) { a.flush2[0] = 1; }},
        {"chunk", [](Args &a) { a.chunk0 = 4096; }},
        {"the last stream's chunk", [](Args &a) { a.chunk2 = 64; }},
        {"raw", [](Args &a) { a.raw0 = true; }},
        {"the last stream's raw", [](Args &a) { a.raw2 = true; }},
        {"env no_rle_multi", [](Args &a) { a.env.no_rle_multi = true; }},
        {"env no_fast_vec", [](Args &a) { a.env.no_fast_vec = true; }},
        {"env fast_no_rounds", [](Args &a) { a.env.fast_no_rounds = true; }},
        {"env no_spec", [](Args &a) { a.env.no_spec = true; }},
        {"env no_fast_multi", [](Args &a) { a.env.no_fast_multi = true; }},
        {"env no_fast_resume", [](Args &a) { a.env.no_fast_resume = true; }},
        {"env no_rle_runs", [](Args &a) { a.env.no_rle_runs = true; }},
        {"env no_resume_rounds", [](Args &a) { a.env.no_resume_rounds = true; }},
        {"env no_live_list", [](Args &a) { a.env.no_live_list = true; }},
        {"env has_fr_ratio", [](Args &a) { a.env.has_fr_ratio = true; }},
        {"env has_fr_chunk", [](Args &a) { a.env.has_fr_chunk = true; }},
        {"env has_fast_chunk", [](Args &a) { a.env.has_fast_chunk = true; }},
        {"env has_spec_len", [](Args &a) { a.env.has_spec_len = true; }},
        {"env has_spec_warm", [](Args &a) { a.env.has_spec_warm = true; }},
        {"env has_spec_min", [](Args &a) { a.env.has_spec_min = true; }},
        {"env has_fast_min_input", [](Args &a) { a.env.has_fast_min_input = true; }},
        {"env spec_len", [](Args &a) { a.env.spec_len = 512; }},
        {"env spec_warm", [](Args &a) { a.env.spec_warm = 1; }},
        {"env fast_chunk", [](Args &a) { a.env.fast_chunk = 65536; }},
        {"env spec_min", [](Args &a) { a.env.spec_min = 65536; }},
        {"env fr_chunk", [](Args &a) { a.env.fr_chunk = 4096; }},
        {"env fast_min_input", [](Args &a) { a.env.fast_min_input = 4194304; }},
        {"env fr_ratio", [](Args &a) { a.env.fr_ratio = 0.5; }},
    };
    // (the walk covers the struct: a field added to PlanKey, PlanKeyWrites or PlanEnv changes one of these sizes, and the
    // list above and the equality are then to be extended with it)
    struct EnvMirror { bool b[16]; int i[3]; int64_t l[3]; double d; };
    static_assert(sizeof(PlanEnv) == sizeof(EnvMirror), "PlanEnv has a field this test does not walk");
    struct WritesMirror { bool present, raw; int chunk; std::vector<int64_t> ends; std::vector<uint8_t> flush; };
    static_assert(sizeof(PlanKeyWrites) == sizeof(WritesMirror), "PlanKeyWrites has a field this test does not walk");
    struct KeyMirror { int i[5]; bool b[4]; std::vector<int64_t> a, c; std::vector<PlanKeyWrites> w; PlanEnv e; };
    static_assert(sizeof(PlanKey) == sizeof(KeyMirror), "PlanKey has a field this test does not walk");
    for (const auto &ch : changes) {
        Args a = base;
        ch.second(a);
        const PlanKey k = key_of(a);
        expect(!plan_key_equal(key_of(base), k) && !plan_key_equal(k, key_of(base)), std::string("a change of ") + ch.first + " makes the keys unequal");
        expect(plan_key_equal(k, key_of(a)), std::string("the key with another ") + ch.first + " equals itself");
    }
    // the paths that are not reused: such a key equals no key
    const std::vector<std::pair<const char *, std::function<void(Args &)>>> barred = {
        {"force_seq 1", [](Args &a) { a.force_seq = 1; }},   {"force_seq 2", [](Args &a) { a.force_seq = 2; }},
        {"incremental", [](Args &a) { a.incremental = true; }}, {"rounds", [](Args &a) { a.rounds = true; }},
        {"forced_lit", [](Args &a) { a.forced_lit = true; }},   {"no_rounds", [](Args &a) { a.no_rounds = true; }},
    };
    for (const auto &ch : barred) {
        Args a = base;
        ch.second(a);
        const PlanKey k = key_of(a);
        expect(!plan_key_reusable(k), std::string(ch.first) + ": not reusable");
        expect(!plan_key_equal(k, key_of(a)) && !plan_key_equal(k, key_of(base)) && !plan_key_equal(key_of(base), k), std::string(ch.first) + ": equals no key");
    }
    // the environment, read: unset gives the defaults, a set switch shows
    {
        const char *names[] = {"ZS_NO_RLE_MULTI", "ZS_NO_FAST_VEC", "ZS_FAST_NO_ROUNDS", "ZS_NO_SPEC", "ZS_NO_FAST_MULTI", "ZS_NO_FAST_RESUME", "ZS_NO_RLE_RUNS",
                               "ZS_NO_RESUME_ROUNDS", "ZS_NO_LIVE_LIST", "ZS_SPEC_LEN", "ZS_SPEC_WARM", "ZS_SPEC_MIN", "ZS_FAST_CHUNK", "ZS_FR_CHUNK", "ZS_FR_RATIO"};
        for (const char *nm : names) unsetenv(nm);
        const PlanEnv clean = plan_env_read();
        expect(plan_env_equal(clean, PlanEnv()), "no switch set: the defaults");
        for (const char *nm : names) {
            setenv(nm, "512", 1);
            expect(!plan_env_equal(clean, plan_env_read()), std::string(nm) + " set: another environment");
            unsetenv(nm);
            expect(plan_env_equal(clean, plan_env_read()), std::string(nm) + " unset again: the first environment");
        }
        setenv("ZS_SPEC_LEN", "512", 1);
        const PlanEnv a = plan_env_read();
        setenv("ZS_SPEC_LEN", "2048", 1);
        expect(!plan_env_equal(a, plan_env_read()), "ZS_SPEC_LEN 512 and 2048 differ");
        unsetenv("ZS_SPEC_LEN");
    }
    printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "PASS", checks, failures);
    return failures ? 1 : 0;
}
