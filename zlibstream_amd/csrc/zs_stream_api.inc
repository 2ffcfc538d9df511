// zs_stream_api.inc -- the z_stream-shaped entry points (included by zs_engine.hip).
//
// Mirrors the caller-visible protocol of Deflate.Compress (Deflate.cs:436-636):
// argument / state checks and their messages (:440-457, :515-526), header
// first (:464-493), output handed out through Flush_pending semantics
// (:828-854), ZSTREAMEND only once everything including the Adler-32 trailer
// has been delivered (:627-635).
//
// When the engine runs.  NoFlush Writes are taken in (copied during the call) and, for a stream that never
// flushes, compressed by the bulk pipeline when Finish arrives -- the fast path.  A Write under FlushMode Partial /
// Sync / Full is a promise to the reader (Deflate.cs:583-613: everything written so far can be decoded from the output
// so far), so it runs the engine at that call: what has been buffered goes through the pipeline as a run that is not the
// stream's end, the literal engine is left suspended in device memory (LitPersist) where Deflate.Compress would return,
// and the bytes up to and including the flush marker are delivered.  From then on the stream is incremental: later
// Writes continue from the suspended engine (input is dropped once consumed: bounded host memory), NoFlush ones a MiB
// at a time.  A NoFlush stream that outgrows 1 GiB of buffered input becomes incremental the same way, so a
// stream has no length limit.  The bytes are the reference's for a caller that runs ZlibOutputStream.WriteCore's loop
// (a fresh output chunk of the same size for every call, ZlibOutputStream.cs:125-168) -- block ends, markers and the
// empty blocks of re-entered flushes included (zs_core.h FlushAcct, carried from run to run).

// std::vector<uint8_t>::resize zero-fills: 64 MiB of output were written twice (5 ms of the Stream API's 44 for a 64 MiB stream)
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    template <class U>
    void construct(U *p) noexcept { ::new ((void *)p) U; }  // default-initialised: nothing written
    template <class U, class... A>
    void construct(U *p, A &&...a) { ::new ((void *)p) U(std::forward<A>(a)...); }
};

// the switches of the tests and the measurements, read once (not per call or per round: getenv walks the environment)
#define ZS_ENV_FLAG(fn, name)                          \
    static bool fn() {                                 \
        static const bool v = getenv(name) != nullptr; \
        return v;                                      \
    }
ZS_ENV_FLAG(no_upload_ahead, "ZS_NO_UPLOAD_AHEAD")
ZS_ENV_FLAG(no_pinned_input, "ZS_NO_PINNED_INPUT")
ZS_ENV_FLAG(no_resume, "ZS_NO_RESUME")
ZS_ENV_FLAG(no_flush_resume, "ZS_NO_FLUSH_RESUME")
ZS_ENV_FLAG(env_debug, "ZS_DEBUG")


// The input a deflate stream has taken in and not yet compressed.  Plain memory, grown by doubling without being filled --
// or, for the one stream of a context that is first to gather 1 MiB, the context's pinned buffer: a copy into pinned memory
// meets no page faults after the buffer's first use (64 MiB of fresh pages cost 8 ms), and what is in it goes to the device
// while the caller is still writing (zs_deflate: `uploaded`).
struct InBuf {
    uint8_t *p = nullptr;
    size_t n = 0, cap = 0;
    bool pinned = false;
    zs_ctx *pin_ctx = nullptr;
    size_t size() const { return n; }
    const uint8_t *data() const { return p; }
    bool grow(size_t want, zs_ctx *c) {
        if (want <= cap) return true;
        size_t ncap = cap ? cap : 4096;
        while (ncap < want) ncap += ncap < ((size_t)256 << 20) ? ncap : ncap / 4;
        constexpr size_t kPinMax = (size_t)512 << 20;  // what a context keeps pinned at most; a stream that gathers more goes on in plain memory
        if (pinned && ncap > kPinMax) {
            (void)hipSetDevice(pin_ctx->device);
            (void)hipStreamSynchronize(pin_ctx->stream);
            uint8_t *q = (uint8_t *)malloc(ncap);
            if (!q) return false;
            if (n) memcpy(q, p, n);
            pin_ctx->pin_io_busy = false;
            p = q, cap = ncap, pinned = false, pin_ctx = nullptr;
            return true;
        }
        if (!pinned && ncap >= ((size_t)1 << 20) && ncap <= kPinMax && c && !c->pin_io_busy && !no_pinned_input()) {
            // move into the context's pinned buffer (grown to what is needed now; it stays with the context)
            (void)hipSetDevice(c->device);
            if (c->pin_io_cap < ncap) {
                if (c->pin_io) (void)hipHostFree(c->pin_io);
                c->pin_io = nullptr, c->pin_io_cap = 0;
                if (hipHostMalloc(&c->pin_io, ncap, hipHostMallocDefault) == hipSuccess) c->pin_io_cap = ncap;
                else (void)hipGetLastError(), c->pin_io = nullptr;
            }
            if (c->pin_io) {
                if (n) memcpy(c->pin_io, p, n);
                free(p);
                p = (uint8_t *)c->pin_io, cap = c->pin_io_cap, pinned = true, pin_ctx = c, c->pin_io_busy = true;
                return true;
            }
        }
        if (pinned) {
            // the pinned buffer is too small: a larger one (transfers out of the old one are waited for first)
            (void)hipSetDevice(pin_ctx->device);
            (void)hipStreamSynchronize(pin_ctx->stream);
            void *np = nullptr;
            if (hipHostMalloc(&np, ncap, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                // back to plain memory
                uint8_t *q = (uint8_t *)malloc(ncap);
                if (!q) return false;
                if (n) memcpy(q, p, n);
                pin_ctx->pin_io_busy = false;
                p = q, cap = ncap, pinned = false, pin_ctx = nullptr;
                return true;
            }
            if (n) memcpy(np, p, n);
            (void)hipHostFree(pin_ctx->pin_io);
            pin_ctx->pin_io = np, pin_ctx->pin_io_cap = ncap;
            p = (uint8_t *)np, cap = ncap;
            return true;
        }
        uint8_t *q = (uint8_t *)realloc(p, ncap);
        if (!q) return false;
        p = q, cap = ncap;
        return true;
    }
    bool append(const uint8_t *src, size_t k, zs_ctx *c) {
        if (!grow(n + k, c)) return false;
        memcpy(p + n, src, k);
        n += k;
        return true;
    }
    void keep_last(size_t keep) {
        if (keep < n) memmove(p, p + (n - keep), keep), n = keep;
    }
    void drop_front(size_t k) {
        if (k >= n) n = 0;
        else memmove(p, p + k, n - k), n -= k;
    }
    const uint8_t *begin() const { return p; }
    const uint8_t *end() const { return p + n; }
    void release() {
        if (pinned) {
            (void)hipSetDevice(pin_ctx->device);
            (void)hipStreamSynchronize(pin_ctx->stream);  // (nothing may still be read out of it for this stream)
            pin_ctx->pin_io_busy = false;
        } else {
            free(p);
        }
        p = nullptr, n = cap = 0, pinned = false, pin_ctx = nullptr;
    }
};

// What an inflate stream has decoded and not yet handed out: read from the device into the context's second pinned buffer
// when that is free (64 MiB into fresh pageable memory: 9 ms; into pinned memory: 2.5), else into plain memory, not zero-filled.
struct OutBuf {
    uint8_t *p = nullptr;
    size_t n = 0, cap = 0;
    bool pinned = false;
    zs_ctx *pin_ctx = nullptr;
    size_t size() const { return n; }
    uint8_t *data() const { return p; }
    const uint8_t *begin() const { return p; }
    const uint8_t *end() const { return p + n; }
    void clear() { n = 0; }
    bool resize(size_t want, zs_ctx *c) {  // (contents are not kept: a decoded piece replaces the one before)
        if (want > cap) {
            release();
            if (want >= ((size_t)1 << 20) && c && !c->pin_out_busy && !no_pinned_input()) {
                (void)hipSetDevice(c->device);
                if (c->pin_out_cap < want) {
                    if (c->pin_out) (void)hipHostFree(c->pin_out);
                    c->pin_out = nullptr, c->pin_out_cap = 0;
                    if (hipHostMalloc(&c->pin_out, want + want / 8, hipHostMallocDefault) == hipSuccess) c->pin_out_cap = want + want / 8;
                    else (void)hipGetLastError(), c->pin_out = nullptr;
                }
                if (c->pin_out) p = (uint8_t *)c->pin_out, cap = c->pin_out_cap, pinned = true, pin_ctx = c, c->pin_out_busy = true;
            }
            if (!p) {
                p = (uint8_t *)malloc(want);
                if (!p) return false;
                cap = want;
            }
        }
        n = want;
        return true;
    }
    void release() {
        if (pinned) pin_ctx->pin_out_busy = false;
        else free(p);
        p = nullptr, n = cap = 0, pinned = false, pin_ctx = nullptr;
    }
};

struct zs_deflate_stream {
    zs_ctx *ctx;
    int level, strategy, window_bits, mem_level, hash_variant, noheader;
    int status;      // 42 INIT, 113 BUSY, 666 FINISH (Deflate.cs:40-42)
    int last_flush;
    const char *msg;
    std::string msg_store;
    InBuf input;
    size_t uploaded = 0;  // leading bytes of `input` that are in the context's device copy already (pinned input, the stream's first run)
    WriteSpec writes;
    std::vector<uint8_t, NoInitAlloc<uint8_t>> output;  // complete zlib stream once compressed
    size_t out_pos, out_end;
    bool compressed;
    int64_t total_in, total_out;
    uint32_t adler;
    // incremental streams
    bool incremental;      // the literal engine is suspended in `persist`
    DevBuf persist;        // LitPersist (device)
    int64_t in_abs;        // stream position of input[0]
    size_t hist;           // leading bytes of `input` the engine has already read (kept: a stored block is copied from them)
    uint32_t carry_byte;   // the bits of the stream's last, incomplete byte (not delivered yet)
    int64_t flush_total_in;  // total_in when the engine last ran for a flush (-1: never): a flush call without input since is the caller's loop coming back ...
    int flush_mode_done;     // ... unless it asks for more than that run gave (Sync, then Full: Deflate.Compress goes on whenever flush > old_flush, Deflate.cs:515)
};

// A run of a stream whose engine is suspended goes back to the bulk pipeline: from the flush the engine stands at (a run of
// one KiB already: the pipeline's launches are ~1.2 ms, the literal engine 2 us a byte at level 6, 0.6 at level 1 -- until late in
// round 5 the line was at 6 KiB and a 4 KiB run took 7.9 ms, a 2 KiB run 4.1; 1.2 now), or -- the engine in the middle of its Writes -- behind a
// window's length of the literal engine
constexpr int64_t kResumeMinBytes = 1 << 10;
inline int64_t resume_min_bytes() {
    static const int64_t v = getenv("ZS_RESUME_MIN") ? atoll(getenv("ZS_RESUME_MIN")) : kResumeMinBytes;
    return v;
}
constexpr int64_t kWarmupMinBytes = 8 << 10;  // (256 KiB while the warm-up was a window's length)
constexpr int64_t kIncRunBytes = 1 << 20;  // an incremental stream runs its NoFlush Writes once this much has gathered
constexpr int64_t kIncBulkRunBytes = 64 << 20;  // ... at the levels whose runs go through the bulk pipeline
// a NoFlush stream whose buffered input outgrows this stops buffering and becomes incremental (ZS_INC_SWITCH_BYTES: tests)
inline int64_t inc_switch_bytes() {
    static const int64_t v = [] {
        const char *e = getenv("ZS_INC_SWITCH_BYTES");
        const long long x = e ? atoll(e) : 0;
        return x > 0 ? (int64_t)x : (int64_t)1 << 30;
    }();
    return v;
}

namespace {
// Adler32.Calculate over the caller's span, on the host: bookkeeping for the
// z_stream `adler` field only (the trailer itself is computed on the device).
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
}  // namespace
#include <immintrin.h>
namespace {
// 32 bytes per step (the reference's own Adler-32 is vectorised the same way, Adler32.cs:82-268): s2 gains 32 s1 + sum (32 - j) b_j.
__attribute__((target("avx2"))) inline uint32_t hsum_avx2(__m256i v) {
    __m128i t = _mm_add_epi32(_mm256_castsi256_si128(v), _mm256_extracti128_si256(v, 1));
    t = _mm_add_epi32(t, _mm_shuffle_epi32(t, 0x4E));
    t = _mm_add_epi32(t, _mm_shuffle_epi32(t, 0xB1));
    return (uint32_t)_mm_cvtsi128_si32(t);
}
__attribute__((target("avx2"))) uint32_t host_adler_avx2(uint32_t adler, const uint8_t *p, size_t n) {
    uint32_t s1 = adler & 0xFFFF, s2 = adler >> 16;
    const __m256i w = _mm256_setr_epi8(32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17, 16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6,
                                       5, 4, 3, 2, 1);
    const __m256i ones = _mm256_set1_epi16(1), zero = _mm256_setzero_si256();
    while (n >= 32) {
        size_t blocks = n / 32;
        if (blocks > 128) blocks = 128;  // 128 x 32 = 4096 < NMAX 5552: no sum overflows before the reduction
        n -= blocks * 32;
        __m256i v1 = zero, v2 = zero, v1run = zero;  // v1: byte sums; v2: weighted sums; v1run: sum of the s1 before each block
        for (size_t b = 0; b < blocks; b++, p += 32) {
            const __m256i x = _mm256_loadu_si256((const __m256i *)p);
            v1run = _mm256_add_epi32(v1run, v1);
            v1 = _mm256_add_epi32(v1, _mm256_sad_epu8(x, zero));                       // 4 x 64-bit lanes, low 32 bits used
            v2 = _mm256_add_epi32(v2, _mm256_madd_epi16(_mm256_maddubs_epi16(x, w), ones));
        }
        const uint64_t sum1 = hsum_avx2(v1), run1 = hsum_avx2(v1run), sum2 = hsum_avx2(v2);
        // every block adds 32 * (s1 before it) + its weighted sum; s1 before block b = s1_0 + (byte sums of the blocks before)
        uint64_t t2 = (uint64_t)s2 + 32ull * ((uint64_t)blocks * s1 + run1) + sum2;
        s1 = (uint32_t)((s1 + sum1) % kAdlerBase);
        s2 = (uint32_t)(t2 % kAdlerBase);
    }
    while (n--) s1 += *p++, s2 += s1;
    s1 %= kAdlerBase, s2 %= kAdlerBase;
    return (s2 << 16) | s1;
}
#define ZS_HOST_ADLER_AVX2 1
#endif

uint32_t host_adler(uint32_t adler, const uint8_t *p, size_t n) {
#ifdef ZS_HOST_ADLER_AVX2
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2 && n >= 64) return host_adler_avx2(adler, p, n);
#endif
    // s1 = sum of bytes, s2 = sum of the running s1: a group of 8 bytes adds 8 * s1 + sum (8 - j) b_j to s2.  Both sums come
    // out of multiplications on the even and the odd bytes spread over 16-bit lanes (no lane can overflow: 4 * 255 * 8).
    uint64_t s1 = adler & 0xFFFF, s2 = adler >> 16;
    const uint64_t m = 0x00FF00FF00FF00FFull;
    while (n) {
        size_t k = n < 4096 ? n : 4096;
        n -= k;
        for (; k >= 8; k -= 8, p += 8) {
            uint64_t x;
            memcpy(&x, p, 8);  // little-endian host: byte j at bits 8 j
            const uint64_t e = x & m, o = (x >> 8) & m;  // bytes 0 2 4 6 / 1 3 5 7 in lanes 0..3
            const uint64_t sum = ((e + o) * 0x0001000100010001ull) >> 48;
            const uint64_t wsum = ((e * 0x0008000600040002ull) >> 48) + ((o * 0x0007000500030001ull) >> 48);
            s2 += 8 * s1 + wsum;
            s1 += sum;
        }
        while (k--) s1 += *p++, s2 += s1;
        s1 %= kAdlerBase, s2 %= kAdlerBase;
    }
    return (uint32_t)((s2 << 16) | s1);
}
}  // namespace

extern "C" {

zs_deflate_stream *zs_deflate_init(zs_ctx *ctx, int level, int strategy, int window_bits, int mem_level, int hash_variant) {
    // Deflate..ctor argument checks (Deflate.cs:241-281)
    int noheader = 0;
    if (level == -1) level = 6;
    if (level == 0) mem_level = 7;
    if (window_bits < 0) noheader = 1, window_bits = -window_bits;
    if (!ctx || mem_level < 1 || mem_level > 9 || window_bits < 9 || window_bits > 15 || level < 0 || level > 9 || strategy < 0 ||
        strategy > 4 || hash_variant < 0 || hash_variant > 1)
        return nullptr;
    zs_deflate_stream *s = new zs_deflate_stream();
    s->ctx = ctx;
    s->level = level, s->strategy = strategy, s->window_bits = window_bits, s->mem_level = mem_level;
    s->hash_variant = hash_variant, s->noheader = noheader;
    s->status = noheader ? 113 : 42;
    s->last_flush = ZS_NO_FLUSH;
    s->msg = nullptr;
    s->out_pos = s->out_end = 0;
    s->compressed = false;
    s->total_in = s->total_out = 0;
    s->adler = 1;
    s->incremental = false;
    s->in_abs = 0;
    s->hist = 0;
    s->carry_byte = 0;
    s->flush_total_in = -1;
    s->flush_mode_done = 0;
    return s;
}

void zs_deflate_end(zs_deflate_stream *s) {
    if (!s) return;
    if (s->persist.p) {
        (void)hipSetDevice(s->ctx->device);
        (void)hipFree(s->persist.p);
    }
    s->input.release();
    delete s;
}
const char *zs_last_message(const zs_deflate_stream *s) { return s ? s->msg : nullptr; }

int zs_deflate(zs_deflate_stream *s, const uint8_t *next_in, int32_t *avail_in, uint8_t *next_out, int32_t *avail_out, int flush,
               uint32_t *adler, int64_t *total_in, int64_t *total_out) {
    if (!s || !avail_in || !avail_out) return ZS_STREAM_ERROR;
    auto sync_out = [&]() {
        if (adler) *adler = s->adler;
        if (total_in) *total_in = s->total_in;
        if (total_out) *total_out = s->total_out;
    };
    if (flush > ZS_FINISH || flush < 0) return ZS_STREAM_ERROR;
    if (next_out == nullptr || (next_in == nullptr && *avail_in != 0) || (s->status == 666 && flush != ZS_FINISH)) {
        s->msg = "stream error";
        return ZS_STREAM_ERROR;
    }
    if (*avail_out == 0) {
        s->msg = "buffer error";
        return ZS_BUF_ERROR;
    }
    if (s->window_bits != 15 || (s->mem_level != 8 && s->level != 0)) {
        s->msg = "only windowBits 15 and memLevel 8 run on the device path";
        return ZS_STREAM_ERROR;
    }
    int old_flush = s->last_flush;
    s->last_flush = flush;
    size_t hdr_skip = s->noheader ? 2 : 0;
    // the 2-byte zlib header is the first pending output (Deflate.cs:464-493)
    if (s->total_in == 0 && s->writes.ends.empty()) s->writes.chunk = *avail_out;  // bufferSize of the caller's WriteCore loop
    if (s->status == 42) {
        s->status = 113;
        unsigned h = zlib_header(s->level);
        s->output.assign({(uint8_t)(h >> 8), (uint8_t)h});
        s->out_pos = 0, s->out_end = 2;
    }
    auto drain = [&]() {
        size_t k = s->out_end - s->out_pos;
        if (k > (size_t)*avail_out) k = (size_t)*avail_out;
        if (k) {
            memcpy(next_out, s->output.data() + s->out_pos, k);
            next_out += k;
            s->out_pos += k;
            *avail_out -= (int32_t)k;
            s->total_out += (int64_t)k;
        }
    };
    bool had_pending = s->out_pos < s->out_end;
    if (had_pending) {
        drain();
        if (*avail_out == 0) {
            s->last_flush = -1;
            sync_out();
            return ZS_OK;
        }
    } else if (*avail_in == 0 && flush <= old_flush && flush != ZS_FINISH) {
        s->msg = "buffer error";
        return ZS_BUF_ERROR;
    }
    if (s->status == 666 && *avail_in != 0) {
        s->msg = "buffer error";
        return ZS_BUF_ERROR;
    }
    // One run of the engine over what has been buffered: `final` = the stream ends here.  A run that is not the end (or
    // continues one) leaves / takes the suspended engine in `persist`; its output is appended to the delivery queue.
    auto run_engine = [&](bool final) -> bool {
        zs_ctx *c = s->ctx;
        if (hipSetDevice(c->device) != hipSuccess) return false;
        const bool legacy = final && !s->incremental;  // the whole stream at once: bulk pipeline, trailer from the device
        int64_t n = (int64_t)s->input.size();
        // every Write under a flush mode adds a block end, a marker and now and then an empty block; a continued run also
        // encodes the block that was in progress (up to 16 383 symbols)
        int64_t cap = zs_deflate_bound(n) + 48 * (int64_t)s->writes.ends.size() + 96 + (s->incremental ? 128 * 1024 : 0);
        s->writes.raw = s->noheader != 0;
        if (!legacy && !s->persist.p) {
            if (!ensure(c, s->persist, sizeof(LitPersist))) return false;
            if (hipMemset(s->persist.p, 0, sizeof(LitPersist)) != hipSuccess) return false;
        }
        // the input on the device: what the Writes have sent ahead (pinned input, first run) plus the rest, else all of it now
        const bool ahead = s->input.pinned && s->uploaded > 0 && s->uploaded <= (size_t)n && c->own_in.cap >= (size_t)n + 256;
        DevBuf &in_dev = ahead ? c->own_in : c->stage_in;
        bool ok = ensure(c, in_dev, (size_t)n + 256) && ensure(c, c->stage_out, (size_t)cap + 256);
        const size_t have = ahead ? s->uploaded : 0;
        if (ok && (size_t)n > have)
            ok = hipMemcpyAsync((uint8_t *)in_dev.p + have, s->input.data() + have, (size_t)n - have, hipMemcpyHostToDevice, c->stream) == hipSuccess;
        s->uploaded = 0;  // (the run consumes the buffer: what stays is history)
        if (s->out_pos == s->out_end) s->output.clear(), s->out_pos = s->out_end = 0;
        else if (s->out_pos > (1u << 20)) {
            s->output.erase(s->output.begin(), s->output.begin() + (ptrdiff_t)s->out_pos);
            s->out_end -= s->out_pos, s->out_pos = 0;
        }
        s->output.resize(s->out_end);
        // one call of the pipeline and its output into the delivery queue; `last`: the stream ends with it
        auto one_call = [&](RunOpts *ro, const WriteSpec &ws, bool last, bool first_of_stream) -> bool {
            const void *din = in_dev.p;
            void *dout = c->stage_out.p;
            int64_t olen = 0;
            int st = 0;
            const auto t0 = std::chrono::steady_clock::now();
            const WriteSpec *const wsp = &ws;
            if (!run_pipeline(c, 1, &din, &n, &dout, &cap, &olen, &st, s->level, s->strategy, s->hash_variant, c->stream, &wsp, !last, ro)) return false;
            if (env_debug())
                fprintf(stderr, "[zs] stream run: %lld bytes, %s, %.2f ms, %lld bytes out\n", (long long)n, !ro ? "whole stream" : ro->resume ? "resumed on the bulk path" : ro->stop_abs >= 0 ? "warm-up" : ro->cont ? "continued" : "first run",
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), (long long)olen);
            if (getenv("ZS_DEBUG") && atoi(getenv("ZS_DEBUG")) > 1) {
                for (int k = 0; k < zs_ctx_stage_count(c); k++)
                    if (zs_ctx_stage_ms(c, k) > 0.05) fprintf(stderr, "[zs]    %-28s %8.3f ms\n", zs_ctx_stage_name(c, k), zs_ctx_stage_ms(c, k));
            }
            // a run that is not the end delivers complete bytes; the bits of the next byte stay with the stream
            const bool partial = ro && !last && (ro->end_bits & 7) != 0;
            // the zlib header (the stream's bytes 0..1) is delivered by the first call; raw streams drop header and trailer.
            // Straight into the delivery queue (no zero fill, no second copy: 27 MB of output cost 8 ms that way)
            const size_t head_skip = first_of_stream ? 2 : 0, tail_skip = last && s->noheader ? 4 : 0;
            const size_t take = (size_t)olen > head_skip + tail_skip ? (size_t)olen - head_skip - tail_skip : 0;
            const size_t at = s->output.size();
            uint8_t carry = 0;
            if (take) {
                s->output.resize(at + take);
                if (hipMemcpy(s->output.data() + at, (const uint8_t *)dout + head_skip, take, hipMemcpyDeviceToHost) != hipSuccess) return false;
            }
            if (partial && hipMemcpy(&carry, (const uint8_t *)dout + olen, 1, hipMemcpyDeviceToHost) != hipSuccess) return false;
            s->out_end = s->output.size();
            s->carry_byte = carry;
            return true;
        };
        auto make_ro = [&](bool fin, bool cont) {
            RunOpts ro;
            ro.final_run = fin, ro.cont = cont, ro.persist = (LitPersist *)s->persist.p, ro.hist = (int64_t)s->hist;
            ro.abs_off = s->in_abs, ro.adler_stream = s->adler, ro.carry_byte = s->carry_byte;
            return ro;
        };
        // A run of a stream whose engine is suspended goes back to the bulk pipeline (zs_engine.hip RunOpts::resume), on the hash
        // chains that engine left (zs_import_chains_kernel): from the flush itself when the engine stands at one -- the run's
        // first pass through the loop reads, as a stream's first one does --, else (a NoFlush stream that outgrew the buffer)
        // from a loop-top no read has touched, where the literal engine stops after a window's length.
        const LevelCfg lvc = level_cfg(s->level);
        bool inner_flush = false;
        for (size_t k = 0; k + 1 < s->writes.flush.size(); k++) inner_flush = inner_flush || s->writes.flush[k] != 0;
        // (levels 1-3, round 5: from a flush only -- the sweeps' stream form starts at p0 on the imported chains; the warm-up route
        // below, a lazy-parse node to resume in, is the slow levels')
        const bool fast_level = lvc.func == 1;
        const bool try_bulk = ok && s->incremental && (lvc.func == 2 || fast_level) && s->strategy != kRle && !inner_flush && !no_resume() &&
                              (int64_t)(n - (int64_t)s->hist) >= resume_min_bytes();
        if (ok && legacy) {
            ok = one_call(nullptr, s->writes, true, true);
        } else if (ok && !try_bulk) {
            RunOpts ro = make_ro(final, s->incremental);
            ok = one_call(&ro, s->writes, final, !s->incremental);
        } else if (ok) {
            LitPersist hp;  // (the scalars in front of the window image)
            ok = hipMemcpy(&hp, s->persist.p, offsetof(LitPersist, window), hipMemcpyDeviceToHost) == hipSuccess;
            bool resumed = false, no_resume = false;
            // the bulk pipeline from buffer position p0 on, if the schedule behind it is one for it; a run that finds it is not
            // after all (zs_core.h kMapPoisonBit: known in the resolve kernel) leaves the engine as it was
            auto resume_from = [&](RunOpts &rb, const WriteSpec &wb) -> bool {
                Geometry g;
                GeoStart gs;
                gs.resume = true, gs.at_read = rb.at_read, gs.p0 = rb.p0, gs.E0 = rb.E0, gs.base0 = rb.base0;
                const std::vector<int64_t> no_ends;
                if (fast_level) {  // one Write behind the flush, every read with a full lookahead (run_pipeline builds the same events)
                    std::vector<ReadEvent> rev;
                    const int64_t one_write[1] = {n};
                    if (rb.base0 < 0 || wb.ends.empty() || !rb.at_read || n - rb.p0 < 2 * kMinLookahead ||
                        !(wb.ends.size() > 1 ? build_read_events(n, wb.ends, rev, true, rb.p0, rb.base0)
                                             : build_read_events(n, std::vector<int64_t>(one_write, one_write + 1), rev, true, rb.p0, rb.base0)))
                        return true;
                } else if (rb.base0 < 0 || wb.ends.empty() || !build_geometry(n, wb.ends.size() > 1 ? wb.ends : no_ends, g, gs)) return true;
                // (the engine's chains must be expressible as links: zs_resume_check_kernel)
                int cannot = 0;
                if (!ensure(c, c->resume_flag, 64) || hipMemsetAsync(c->resume_flag.p, 0, 4, c->stream) != hipSuccess) return false;
                hipLaunchKernelGGL(zs_resume_check_kernel, dim3(32), dim3(1024), 0, c->stream, (const LitPersist *)s->persist.p, rb.p0 + s->in_abs,
                                   (int *)c->resume_flag.p);
                if (hipMemcpyAsync(&cannot, c->resume_flag.p, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                    hipStreamSynchronize(c->stream) != hipSuccess)
                    return false;
                if (cannot) {
                    no_resume = true;
                    return true;
                }
                if (!ensure(c, c->persist_bak, sizeof(LitPersist)) ||
                    hipMemcpy(c->persist_bak.p, s->persist.p, sizeof(LitPersist), hipMemcpyDeviceToDevice) != hipSuccess)
                    return false;
                c->resume_poisoned = false;
                const size_t out_before = s->output.size();
                if (one_call(&rb, wb, final, false)) {
                    resumed = true;
                    return true;
                }
                if (!c->resume_poisoned) return false;
                s->output.resize(out_before), s->out_end = s->output.size();
                return hipMemcpy(s->persist.p, c->persist_bak.p, sizeof(LitPersist), hipMemcpyDeviceToDevice) == hipSuccess;
            };
            auto writes_from = [&](int64_t from_abs) {  // the Writes that end at or behind a stream position, in buffer positions
                WriteSpec wb;
                wb.chunk = s->writes.chunk, wb.raw = s->writes.raw;
                for (size_t k = 0; k < s->writes.ends.size(); k++)
                    if (s->writes.ends[k] >= from_abs) wb.ends.push_back(s->writes.ends[k] - s->in_abs), wb.flush.push_back(s->writes.flush[k]);
                return wb;
            };
            const int64_t F = s->in_abs + (int64_t)s->hist;
            if (ok && hp.lookahead == 0 && hp.match_available == 0 && hp.pending_syms == 0 && hp.avail_end == F && hp.base + hp.strstart == F &&
                hp.block_start_abs == F && !no_flush_resume()) {
                // the engine stands where a flush left it (Deflate.cs:583-613): nothing read ahead, nothing pending, the block
                // closed.  The bulk pipeline goes on from that very position -- its first pass through the loop reads, as a
                // stream's first one does -- with the chains the engine left (zs_import_chains_kernel)
                RunOpts rb = make_ro(final, false);
                rb.resume = true, rb.at_read = true;
                rb.p0 = rb.E0 = F - s->in_abs, rb.base0 = hp.base - s->in_abs, rb.start_block = rb.p0, rb.start_syms = 0, rb.slot = 0;
                ok = resume_from(rb, writes_from(F + 1));
            }
            if (ok && !resumed && (no_resume || fast_level || (int64_t)(n - (int64_t)s->hist) < kWarmupMinBytes)) {
                RunOpts ro = make_ro(final, true);
                ok = one_call(&ro, s->writes, final, false);
            } else if (ok && !resumed) {
                // ... or from where the literal engine stops after a window's length (it is in the middle of the stream's Writes
                // anyhow: a NoFlush stream that outgrew the buffer, a schedule the bulk path does not begin with)
                RunOpts ra = make_ro(false, true);
                // (a KiB of the literal engine, 3 ms -- until late in round 5 a window's length, 65 ms in front of every run: what the bulk path
                // needs is a loop-top with a full lookahead that no read has touched, and the engine stops at the first one behind stop_abs)
                static const int64_t warm = getenv("ZS_WARMUP_BYTES") ? atoll(getenv("ZS_WARMUP_BYTES")) : 1024;
                ra.stop_abs = F + warm;
                ok = one_call(&ra, s->writes, false, false);
                if (ok) ok = hipMemcpy(&hp, s->persist.p, offsetof(LitPersist, window), hipMemcpyDeviceToHost) == hipSuccess;
                if (ok && hp.stopped) {
                    RunOpts rb = make_ro(final, false);
                    rb.resume = true;
                    rb.p0 = hp.base + hp.strstart - s->in_abs, rb.E0 = hp.avail_end - s->in_abs, rb.base0 = hp.base - s->in_abs;
                    rb.start_block = hp.block_start_abs - s->in_abs, rb.start_syms = (uint32_t)hp.pending_syms;
                    rb.slot = hp.match_available == 0 ? 0 : hp.match_length < kMinMatch ? 256 + kL : hp.good_prev ? 256 + kXK4 : 256 + kXK;
                    // the Write the engine is in and the ones behind it
                    ok = resume_from(rb, writes_from(hp.avail_end));
                }
                if (ok && !resumed && (hp.stopped || final)) {
                    // (the schedule behind the stop is not one for the bulk path: on with the literal engine; an engine that
                    // never stopped -- Writes of a few bytes -- has taken in all of them: Finish is what is left)
                    RunOpts rc = make_ro(final, true);
                    rc.mid_write = hp.stopped != 0;
                    WriteSpec wc;
                    wc.chunk = s->writes.chunk, wc.raw = s->writes.raw;
                    for (size_t k = 0; k < s->writes.ends.size(); k++)
                        if (hp.stopped && s->writes.ends[k] >= hp.avail_end) wc.ends.push_back(s->writes.ends[k]), wc.flush.push_back(s->writes.flush[k]);
                    ok = one_call(&rc, wc, final, false);
                }
            }
        }
        if (!ok) {
            s->msg_store = "device deflate failed: " + c->err;
            s->msg = s->msg_store.c_str();
            return false;
        }
        // everything has been read; the last 64 KiB stay (a later stored block may start in them, Deflate.cs:953)
        const size_t keep = final ? 0 : std::min<size_t>((size_t)n, (size_t)kWindowSize);
        s->in_abs += n - (int64_t)keep;
        s->input.keep_last(keep);
        s->hist = keep;
        s->writes.ends.clear(), s->writes.flush.clear();
        if (final) {
            s->compressed = true;
            s->input.release();
        } else {
            s->incremental = true;
        }
        return true;
    };
    if (*avail_in > 0 && (int64_t)s->input.size() + *avail_in > (int64_t)0x7FFFFFFF - 1024) {
        // the device pipeline indexes one run with 32-bit positions: what is buffered goes first, as a run of its own
        if (s->input.size() == s->hist || !run_engine(false)) {
            if (s->input.size() == s->hist) s->msg = "a single Write beyond 2 GiB - 65 KiB is not supported by the device path";
            s->last_flush = old_flush;
            return s->input.size() == s->hist ? ZS_MEM_ERROR : ZS_STREAM_ERROR;  // *avail_in untouched
        }
        // the run keeps up to 64 KiB of history in front of the new Write: the limit holds for the two together
        if ((int64_t)s->input.size() + *avail_in > (int64_t)0x7FFFFFFF - 1024) {
            s->msg = "a single Write beyond 2 GiB - 65 KiB is not supported by the device path";
            s->last_flush = old_flush;
            return ZS_MEM_ERROR;  // *avail_in untouched
        }
    }
    const bool is_flush = flush == ZS_PARTIAL_FLUSH || flush == ZS_SYNC_FLUSH || flush == ZS_FULL_FLUSH;
    bool new_write = false;
    if (*avail_in > 0) {
        // a flush promises the reader everything written so far: NoFlush Writes that are waiting go through the pipeline as
        // a run of their own first (the bulk path, where their schedule allows it), the flushing Write continues from there
        if (is_flush && !s->writes.ends.empty() && !s->writes.flushing() && (int64_t)(s->input.size() - s->hist) >= kIncRunBytes && !run_engine(false))
            return ZS_STREAM_ERROR;
        // ReadBuffer (ZlibStream.cs:197-222): copy during the call, update Adler / TotalIn
        if (!s->input.append(next_in, (size_t)*avail_in, s->ctx)) {
            s->msg = "insufficient memory";
            return ZS_MEM_ERROR;
        }
        // a stream that has not run yet and sits in pinned memory sends its bytes ahead: the transfer runs beside the checksum
        // below and the caller's next Writes, and Finish finds the input on the device
        if (s->input.pinned && !s->incremental && s->in_abs == 0 && s->input.size() - s->uploaded >= ((size_t)256 << 10) && !no_upload_ahead()) {
            zs_ctx *c = s->ctx;
            if (hipSetDevice(c->device) == hipSuccess) {
                if (c->own_in.cap < s->input.cap + 256) {  // (sized like the host buffer: it grows when that one does -- a new buffer, whatever its address)
                    (void)ensure(c, c->own_in, s->input.cap + 256);
                    s->uploaded = 0;
                }
                if (c->own_in.cap >= s->input.size() + 256 &&
                    hipMemcpyAsync((uint8_t *)c->own_in.p + s->uploaded, s->input.data() + s->uploaded, s->input.size() - s->uploaded, hipMemcpyHostToDevice, c->stream) == hipSuccess)
                    s->uploaded = s->input.size();
                else
                    (void)hipGetLastError();
            }
        }
        if (!s->noheader) s->adler = host_adler(s->adler, next_in, (size_t)*avail_in);
        s->total_in += *avail_in;
        *avail_in = 0;
        s->writes.ends.push_back(s->in_abs + (int64_t)s->input.size());
        s->writes.flush.push_back(flush == ZS_FINISH ? 0 : (uint8_t)flush);
        new_write = true;
    } else if (is_flush && !s->compressed && !(had_pending && s->incremental) && (s->total_in != s->flush_total_in || flush > s->flush_mode_done)) {
        // (a call that found output of an earlier run pending is the caller's loop coming back for the rest of it -- and so is
        // one that finds nothing pending and nothing written since the engine ran for a flush: the call before handed out the
        // last of that run's output and filled its chunk with it.  Where the reference's own chunks fill at a flush it
        // enters the block function again and adds an empty block; the offsets kernel has put those into the stream already,
        // following the reference's chunking Write by Write (zs_core.h FlushAcct), which is not the one this delivery has when
        // NoFlush Writes waited for the flush.)
        // a flush call without input: the block function runs with what is left and closes the block
        s->writes.ends.push_back(s->in_abs + (int64_t)s->input.size());
        s->writes.flush.push_back((uint8_t)flush);
        new_write = true;
    }
    if (flush != ZS_FINISH) {
        const int64_t buffered = (int64_t)(s->input.size() - s->hist);
        // (behind a flush the slow levels go back to the bulk pipeline, which wants long runs: NoFlush Writes wait as they do
        // in front of the first run; the other levels stay with the literal engine and run as the Writes come)
        const bool bulk_level = level_cfg(s->level).func >= 1 && s->strategy != kRle && !no_resume();  // (levels 1-3 too, since round 5)
        // (64 MiB saturate the bulk pipeline: an incremental stream does not hold more than that back -- the reference hands
        // out compressed bytes as its pending buffer fills)
        const bool run_now = (is_flush && new_write) || (s->incremental && new_write && buffered >= (bulk_level ? std::min<int64_t>(inc_switch_bytes(), kIncBulkRunBytes) : kIncRunBytes)) ||
                             (!s->incremental && buffered > inc_switch_bytes());
        if (run_now) {
            if (!run_engine(false)) return ZS_STREAM_ERROR;
            if (is_flush && new_write) s->flush_total_in = s->total_in, s->flush_mode_done = flush;
            drain();
            if (*avail_out == 0) s->last_flush = -1;  // more is pending: the caller comes again (Deflate.cs:505-514)
        }
        sync_out();
        return ZS_OK;
    }
    if (!s->compressed) {
        s->status = 666;
        if (!run_engine(true)) return ZS_STREAM_ERROR;
    }
    drain();
    sync_out();
    return s->out_pos < s->out_end ? ZS_OK : ZS_STREAM_END;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// zs_inflate: what ZLibStream.Inflate(FlushMode) binds to (ZlibStream.cs:119-122 -> Inflate.Decompress,
// Inflate.cs:103-357), driven by ZlibInputStream.ReadCore (ZlibInputStream.cs:133-186): 8 KiB input chunks while
// BaseStream has data, then calls with no input.  The engine decodes whole streams, so it takes the chunks in
// (ZOK, no output yet), decodes on the GPU at the first call that brings no input -- the caller's signal that the
// compressed data is complete -- and serves the output from then on; ZSTREAMEND with the last byte.  An input that is
// not a complete stream at that point is ZBUFERROR ("buffer error"), which is what the managed engine returns when it
// cannot make progress; corrupt data gives the reference's ZDATAERROR messages.

struct zs_inflate_stream {
    int64_t next_probe = 1 << 20;  // buffered bytes at which the stream's end is looked for next
    int64_t last_probe_size = -1;  // buffered bytes at the last look
    zs_ctx *ctx;
    const char *msg;
    std::string msg_store;
    InBuf input;
    size_t uploaded = 0;  // leading bytes of `input` that are in the context's device copy (pinned input; sent as they arrive)
    OutBuf output;
    size_t out_pos;
    bool decoded, ended;
    int64_t total_in, total_out;
    uint32_t adler;
    // a stream that is decoded as it arrives (the caller asked for output before the stream's end was there): input[0]'s bit
    // `bit_off` is where the next block begins, `hist` the last <= 32 768 bytes delivered so far, `adler` the checksum so far
    bool pieces = false;
    int bit_off = 0;
    std::vector<uint8_t> hist;
    DevBuf hist_dev;
    std::vector<uint8_t> surplus;  // what the caller fed behind the stream's end before the end was seen (zs_inflate_surplus)
};

// the bounded form: a stream that is fed and fed without its caller asking for output is decoded up to its last complete
// block whenever this much has been buffered
constexpr int64_t kInfPieceBytesDefault = 64 << 20;
// (ZS_INF_PIECE_BYTES: the tests reach the bounded form with a few hundred KiB)
static int64_t inf_piece_bytes() {
    static const int64_t v = [] {
        const char *e = getenv("ZS_INF_PIECE_BYTES");
        const long long x = e ? atoll(e) : 0;
        return (int64_t)(x >= 4096 ? x : kInfPieceBytesDefault);
    }();
    return v;
}

extern "C" {

zs_inflate_stream *zs_inflate_init(zs_ctx *ctx, int window_bits) {
    // Inflate..ctor (Inflate.cs:76-96): 8..15, negative = raw; only zlib-wrapped streams with the full window run here
    if (!ctx || window_bits != 15) return nullptr;
    zs_inflate_stream *s = new zs_inflate_stream();
    s->ctx = ctx;
    s->msg = nullptr;
    s->out_pos = 0;
    s->decoded = s->ended = false;
    s->total_in = s->total_out = 0;
    s->adler = 1;
    return s;
}

void zs_inflate_end(zs_inflate_stream *s) {
    if (!s) return;
    if (s->hist_dev.p && hipSetDevice(s->ctx->device) == hipSuccess) (void)hipFree(s->hist_dev.p);
    s->input.release();
    s->output.release();
    delete s;
}
const char *zs_inflate_message(const zs_inflate_stream *s) { return s ? s->msg : nullptr; }

// Bytes the caller fed behind the stream's trailer in calls BEFORE the one that found the stream's end (that call's own
// surplus stays in its *avail_in): a caller with data behind the zlib stream -- concatenated streams, a container's
// records -- takes them from here.  Returns the count; *p points into the stream object (valid until zs_inflate_end).
int64_t zs_inflate_surplus(const zs_inflate_stream *s, const uint8_t **p) {
    if (!s) return 0;
    if (p) *p = s->surplus.data();
    return (int64_t)s->surplus.size();
}

int zs_inflate(zs_inflate_stream *s, const uint8_t *next_in, int32_t *avail_in, uint8_t *next_out, int32_t *avail_out, int flush,
               uint32_t *adler, int64_t *total_in, int64_t *total_out) {
    (void)flush;  // Inflate.Decompress only uses it to pick the "no progress" return code
    if (!s || !avail_in || !avail_out || (next_in == nullptr && *avail_in != 0)) return ZS_STREAM_ERROR;
    auto sync_out = [&]() {
        if (adler) *adler = s->adler;
        if (total_in) *total_in = s->total_in;
        if (total_out) *total_out = s->total_out;
    };
    if (s->ended) {
        sync_out();
        return ZS_STREAM_END;
    }
    const int32_t this_call = *avail_in;
    // the first in_len bytes of the buffered input on the device: the copy that went ahead (completed by what is missing), else
    // a fresh copy in the context's staging buffer
    auto stage_input = [&](int64_t in_len) -> const void * {
        zs_ctx *c = s->ctx;
        if (s->input.pinned && s->uploaded > 0 && c->own_in.cap >= (size_t)in_len + 256) {
            if ((size_t)in_len > s->uploaded) {
                if (hipMemcpyAsync((uint8_t *)c->own_in.p + s->uploaded, s->input.data() + s->uploaded, (size_t)in_len - s->uploaded, hipMemcpyHostToDevice, c->stream) != hipSuccess)
                    return nullptr;
                s->uploaded = (size_t)in_len;
            }
            return c->own_in.p;
        }
        if (!ensure(c, c->stage_in, (size_t)in_len + 256)) return nullptr;
        if (in_len && hipMemcpyAsync(c->stage_in.p, s->input.data(), (size_t)in_len, hipMemcpyHostToDevice, c->stream) != hipSuccess) return nullptr;
        return c->stage_in.p;
    };
    // Has the stream's end arrived in what is buffered?  The block finder, the measuring pass and the chain of blocks, nothing
    // decoded; returns the stream's length with its trailer, or 0
    auto look_for_end = [&]() -> int64_t {
        zs_ctx *c = s->ctx;
        int64_t in_len = (int64_t)s->input.size(), used = 0;
        const auto t0 = std::chrono::steady_clock::now();
        bool ok = hipSetDevice(c->device) == hipSuccess;
        const void *din_probe = ok ? stage_input(in_len) : nullptr;
        ok = ok && din_probe != nullptr;
        if (ok) {
            const void *din = din_probe;
            void *dout = nullptr;
            int64_t cap0 = 0, olen0 = 0;
            int st0 = 0;
            std::vector<int> one(1, 0), rest;
            c->inf_probe = &used;
            ok = run_inflate_par(c, one, &din, &in_len, &dout, &cap0, &olen0, &st0, c->stream, rest);
            c->inf_probe = nullptr;
        }
        s->last_probe_size = in_len;
        static const bool dbg = getenv("ZS_DEBUG") != nullptr;
        if (dbg)
            fprintf(stderr, "[zs] inflate: looked for the stream's end in %lld bytes: %s, %.2f ms\n", (long long)in_len,
                    ok && used > 0 ? "found" : "not there", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        return ok && used > 0 ? used : 0;
    };
    if (!s->decoded && s->out_pos == s->output.size()) {
        zs_ctx *c = s->ctx;
        const int64_t limit = (int64_t)0x7FFFFFFF - 1024;
        int64_t stream_len = 0;  // > 0: the stream's end has arrived -- its length with the trailer
        bool piece_now = false;
        if (*avail_in > 0) {
            if ((int64_t)s->input.size() + *avail_in > limit) {
                s->msg = "input beyond 2 GiB - 1 KiB per stream is not supported by the device path";
                return ZS_MEM_ERROR;  // *avail_in untouched
            }
            if (!s->input.append(next_in, (size_t)*avail_in, c)) {
                s->msg = "insufficient memory";
                return ZS_MEM_ERROR;
            }
            s->total_in += *avail_in;
            *avail_in = 0;
            // pinned input goes to the device as it arrives: the looks for the stream's end and the decode find it there
            if (s->input.pinned && s->input.size() - s->uploaded >= ((size_t)256 << 10) && !no_upload_ahead() && hipSetDevice(c->device) == hipSuccess) {
                if (c->own_in.cap < s->input.cap + 256) {  // (a new buffer, whatever its address)
                    (void)ensure(c, c->own_in, s->input.cap + 256);
                    s->uploaded = 0;
                }
                if (c->own_in.cap >= s->input.size() + 256 &&
                    hipMemcpyAsync((uint8_t *)c->own_in.p + s->uploaded, s->input.data() + s->uploaded, s->input.size() - s->uploaded, hipMemcpyHostToDevice, c->stream) == hipSuccess)
                    s->uploaded = s->input.size();
                else
                    (void)hipGetLastError();
            }
            // Has the stream's end arrived?  Inflate.Decompress ends with the final block's trailer whatever follows in the
            // caller's stream (Inflate.cs:292-357): the end is looked for in what has been buffered -- the block finder, the
            // measuring pass and the chain of blocks, nothing decoded -- whenever the buffered bytes have quadrupled since the
            // last look (all the looks together cost a third of a pass over the input; doubling -- seven looks for 64 MiB --
            // cost the Stream API 8.6 ms in round 3), from 1 MiB on (1-2 ms per look); a shorter
            // stream is decoded when its caller runs out of input, like a longer one whose end never shows.
            if (!s->pieces && (int64_t)s->input.size() >= s->next_probe && (int64_t)s->input.size() >= kParMinInput) {
                stream_len = look_for_end();
                s->next_probe = 4 * (int64_t)s->input.size();
            }
            if (stream_len == 0) {
                // nothing is decoded while the caller still brings input -- unless so much has been buffered that the
                // stream has to be taken piece by piece (bounded memory for a stream of any length)
                if ((int64_t)s->input.size() < inf_piece_bytes()) {
                    sync_out();
                    return ZS_OK;
                }
                piece_now = true;
            }
        }
        // The stream's end is there, or the caller has run out of input and wants what the bytes so far decode to
        // (ZlibInputStream.ReadCore: a Read behind a writer's flush, ZlibInputStream.cs:133-186; Inflate.Decompress produces
        // output as input arrives, Inflate.cs:103-357): a whole stream takes the block-parallel decoder; anything else is
        // decoded up to its last complete block -- a flush ends on one (Deflate.cs:583-613) -- and goes on from there with
        // the next input.
        bool whole_done = false;
        // (a long stream whose end has not been seen is looked at first: without its end the block-parallel decode's work would be
        // thrown away and the pieces decode the same bytes again)
        if (!s->pieces && !piece_now && stream_len == 0 && (int64_t)s->input.size() >= kParMinInput && s->last_probe_size != (int64_t)s->input.size())
            stream_len = look_for_end();
        if (!s->pieces && !piece_now && stream_len > 0) {
            int64_t in_len = stream_len > 0 ? stream_len : (int64_t)s->input.size(), out_len = 0;
            int st = 0;
            uint32_t ad = 1;
            bool ok = hipSetDevice(c->device) == hipSuccess;
            const void *din_whole = ok ? stage_input(in_len) : nullptr;
            ok = ok && din_whole != nullptr;
            int64_t cap = std::min<int64_t>(std::max<int64_t>(in_len * 8, 1 << 20), limit);
            bool full = false;
            c->inf_used.assign(1, 0);
            // The decoded size is not known up front: start from a generous bound and grow on ZBUFERROR (a deflate stream
            // expands by at most ~1032x), up to the device path's limit.
            while (ok) {
                if (!ensure(c, c->stage_out, (size_t)cap + 256)) {
                    ok = false;
                    break;
                }
                const void *din = din_whole;
                void *dout = c->stage_out.p;
                run_inflate(c, 1, &din, &in_len, &dout, &cap, &out_len, &st, c->stream, &ad);
                // ZBUFERROR is both "input ends inside the stream" and "output is full"; the decoder stops where it is, so a
                // full output shows as a length within one match of the capacity
                full = st == ZS_BUF_ERROR && out_len + kMaxMatch >= cap;
                if (!full || cap >= limit) break;
                cap = std::min<int64_t>(cap * 4, limit);
            }
            const bool truncated = ok && st == ZS_BUF_ERROR && !full;  // not the whole stream yet: piece by piece from here
            if (!truncated) {
                if (!ok || st != ZS_STREAM_END) {
                    s->msg_store = !ok ? "device inflate failed: " + c->err
                                       : full ? "output beyond 2 GiB - 1 KiB per stream is not supported by the device path" : c->err;
                    s->msg = s->msg_store.c_str();
                    s->output.clear();
                    sync_out();
                    return !ok ? ZS_STREAM_ERROR : (st != ZS_OK && st != ZS_STREAM_END ? st : ZS_DATA_ERROR);
                }
                s->out_pos = 0;
                if (!s->output.resize((size_t)out_len, c) || (out_len && hipMemcpy(s->output.data(), c->stage_out.p, (size_t)out_len, hipMemcpyDeviceToHost) != hipSuccess)) {
                    s->msg = "stream error";
                    return ZS_STREAM_ERROR;
                }
                // the bytes behind the trailer are not this stream's: total_in is the stream's length; what this call brought
                // of them stays with the caller (*avail_in), as with the managed engine, which stops reading at the trailer;
                // what earlier calls brought is kept for zs_inflate_surplus
                const int64_t used = !c->inf_used.empty() && c->inf_used[0] > 0 ? c->inf_used[0] : (int64_t)s->input.size();
                const int64_t over = (int64_t)s->input.size() - used;
                if (over > 0) {
                    const int64_t back = std::min<int64_t>(over, this_call);
                    *avail_in = (int32_t)back;
                    s->surplus.assign(s->input.begin() + used, s->input.end() - back);
                    s->total_in -= over;
                }
                s->decoded = true;
                s->input.release(), s->uploaded = 0;
                s->adler = ad;  // z_stream.adler after a finished inflate (Inflate.cs:339): computed on the device with the trailer check
                whole_done = true;
            }
        }
        if (!whole_done) {
            // ---- a piece: the complete blocks of what is buffered
            const int64_t in_len = (int64_t)s->input.size();
            const int have = (int)s->hist.size();
            int64_t out_len = 0, good = 0, used = 0;
            int st = ZS_OK;
            uint32_t stored = 0;
            bool ok = hipSetDevice(c->device) == hipSuccess && (have == 0 || ensure(c, s->hist_dev, 32768 + 256));
            const void *din_piece = ok ? stage_input(in_len) : nullptr;
            ok = ok && din_piece != nullptr;
            if (ok && have) ok = hipMemcpy(s->hist_dev.p, s->hist.data(), (size_t)have, hipMemcpyHostToDevice) == hipSuccess;
            int64_t cap = std::min<int64_t>(std::max<int64_t>(in_len * 8, 1 << 20), limit);
            bool full = false;
            while (ok) {
                if (!ensure(c, c->stage_out, (size_t)cap + 256)) {
                    ok = false;
                    break;
                }
                ok = run_inflate_piece(c, din_piece, in_len, !s->pieces, (int64_t)s->bit_off, s->hist_dev.p, have, c->stage_out.p, cap, &out_len, &good,
                                       &used, &st, &stored, c->stream);
                full = ok && st == ZS_BUF_ERROR;  // (a piece's only buffer error is a full output)
                if (!full || cap >= limit) break;
                cap = std::min<int64_t>(cap * 4, limit);
            }
            if (!ok || (st != ZS_OK && st != ZS_STREAM_END)) {
                s->msg_store = !ok ? "device inflate failed: " + c->err
                                   : full ? "output beyond 2 GiB - 1 KiB per piece is not supported by the device path" : c->err;
                s->msg = s->msg_store.c_str();
                sync_out();
                return !ok ? ZS_STREAM_ERROR : st;
            }
            s->out_pos = 0;
            if (!s->output.resize((size_t)out_len, c) || (out_len && hipMemcpy(s->output.data(), c->stage_out.p, (size_t)out_len, hipMemcpyDeviceToHost) != hipSuccess)) {
                s->msg = "stream error";
                return ZS_STREAM_ERROR;
            }
            s->adler = host_adler(s->adler, s->output.data(), (size_t)out_len);
            // the window behind the piece: the last 32 KiB of everything delivered
            if (out_len >= kWSize) {
                s->hist.assign(s->output.end() - kWSize, s->output.end());
            } else if (out_len > 0) {
                s->hist.insert(s->hist.end(), s->output.begin(), s->output.end());
                if (s->hist.size() > (size_t)kWSize) s->hist.erase(s->hist.begin(), s->hist.end() - kWSize);
            }
            if (st == ZS_STREAM_END) {
                if (stored != s->adler) {  // Inflate.cs:300-345
                    s->msg = "incorrect data check";
                    s->output.clear();
                    sync_out();
                    return ZS_DATA_ERROR;
                }
                const int64_t over = in_len - used;
                if (over > 0) {
                    const int64_t back = std::min<int64_t>(over, this_call);
                    *avail_in = (int32_t)back;
                    s->surplus.assign(s->input.begin() + used, s->input.end() - back);
                    s->total_in -= over;
                }
                s->decoded = true;
                s->input.release(), s->uploaded = 0;
            } else {
                // the stream goes on: what the complete blocks took leaves the buffer
                if (good > 0) {  // (the header, at least, is behind the stream: pieces from here on)
                    s->pieces = true;
                    s->input.drop_front((size_t)(good >> 3)), s->uploaded = 0;
                    s->bit_off = (int)(good & 7);
                }
                if (out_len == 0 && this_call == 0) {  // no input, nothing new to give: Inflate.Decompress's "no progress"
                    s->msg = "buffer error";
                    sync_out();
                    return ZS_BUF_ERROR;
                }
            }
        }
    }
    if (*avail_out == 0) {
        sync_out();
        if (this_call > 0 && *avail_in < this_call) return ZS_OK;  // (the call took input: progress; input left where it was is none)
        s->msg = "buffer error";
        return ZS_BUF_ERROR;
    }
    size_t k = s->output.size() - s->out_pos;
    if (k > (size_t)*avail_out) k = (size_t)*avail_out;
    if (k) {
        memcpy(next_out, s->output.data() + s->out_pos, k);
        s->out_pos += k;
        *avail_out -= (int32_t)k;
        s->total_out += (int64_t)k;
    }
    sync_out();
    if (s->out_pos == s->output.size()) {
        if (s->decoded) {
            s->ended = true;
            s->output.release(), s->out_pos = 0;  // (the context's pinned buffer is the next stream's)
            return ZS_STREAM_END;
        }
        s->output.clear();  // a piece is through; the next call decodes the next
        s->out_pos = 0;
    }
    return ZS_OK;
}

}  // extern "C"

