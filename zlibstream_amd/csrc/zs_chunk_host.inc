// zs_chunk_host.inc -- host side of the chunked-array calls of include/zsgpu.h: the chunks of HDF5 / NetCDF-4 datasets and
// Zarr v2 arrays (shuffle in front of deflate) from host memory decoded on the device into arrays, arrays that lie there
// written as chunks, and the shuffle filter alone.  Part of zs_engine.hip's translation unit, behind zs_wrap_host.inc, whose
// container calls it calls; the flat-list runner (png_run_list) and the KC job runner (Crc32Job) are zs_png_host.inc's; the
// geometry is zs_chunk.h's, the kernels (KN) zs_chunk.hip's.

namespace {
static_assert(sizeof(zs_chunk_grid) == sizeof(ChunkGrid) && offsetof(zs_chunk_grid, chunk) == offsetof(ChunkGrid, chunk) && offsetof(zs_chunk_grid, fill) == offsetof(ChunkGrid, fill),
              "zs_chunk_grid mirrors ChunkGrid");
static_assert(sizeof(ChunkJob) % 8 == 0 && sizeof(ChunkGeom) % 8 == 0, "the jobs lie in front of the item list, the geometries behind it");
static_assert(ZS_CHUNK_STORED == kChunkStored && ZS_CHUNK_UNSHUFFLED == kChunkUnshuffled && ZS_CHUNK_SKIP == kChunkSkip && ZS_CHUNK_ABSENT == kChunkAbsent, "the flags are zs_chunk.h's");

constexpr PngGrid kChunkGrid{kPngSlice, kChunkItemsPerWg, 64};
enum ChunkMode { kChunkPlace, kChunkGather, kChunkSurvey };

// One KN launch: the arrays' geometries, the chunks, and the flat list of their items.
struct ChunkSet {
    std::vector<ChunkGeom> geoms;
    std::vector<ChunkJob> jobs;
    PngOffsets items;
    bool full = false;  // the items are those of the gather kernel
    int geom(const ChunkGrid &g) {
        geoms.push_back(chunk_geom(g));
        return (int)geoms.size() - 1;
    }
    // chunk c of grid g (geometry k): its bytes at `bytes`, the array at `arr`
    void chunk(const ChunkGrid &g, int k, int64_t c, const void *bytes, const void *arr, int flags) {
        ChunkJob jb;
        const int64_t origin = chunk_place_of(g, c, jb.ext);
        jb.chunk = (uint8_t *)bytes, jb.arr = (uint8_t *)arr + origin * g.elem_size, jb.geom = k, jb.flags = flags;
        jobs.push_back(jb);
        items.add(chunk_item_count(geoms[(size_t)k], jb.ext, full));
    }
};

bool chunk_items_ok(zs_ctx *c, int64_t total) {
    if (total <= 0x7FFFFFFF) return true;
    c->err = "stream error: more than 2^31 - 1 stretches of rows in one call (split the batch)";
    return false;
}

// KN over the set on `s` (png_run_list: one wait, for the upload).  The survey: a record per item into png[kBufChunkRec],
// folded to a byte per chunk behind the records, which `flags` receives (one more wait).
bool chunk_run(zs_ctx *c, ChunkSet &set, ChunkMode mode, hipStream_t s, bool *no_memory, double *ms, std::vector<uint8_t> *flags = nullptr) {
    *no_memory = false;
    const int m = (int)set.jobs.size();
    if (m == 0) return true;
    if (!chunk_items_ok(c, set.items.total)) return false;
    const size_t n_rec = ((size_t)set.items.total + 255) & ~(size_t)255;
    if (mode == kChunkSurvey && !ensure(c, c->png[kBufChunkRec], n_rec + (size_t)m)) {
        *no_memory = true;
        return false;
    }
    uint8_t *d_rec = (uint8_t *)c->png[kBufChunkRec].p;
    const size_t b_job = sizeof(ChunkJob) * (size_t)m, b_off = set.items.bytes(true);
    const int32_t *d_off = nullptr;
    if (!png_run_list(c, c->png[kBufChunkDesc], {{set.jobs.data(), b_job}, {set.geoms.data(), sizeof(ChunkGeom) * set.geoms.size()}}, set.items, 0, kChunkGrid, s, no_memory, ms,
                      [&](dim3 grid, dim3 block, uint8_t *d, int64_t first) {
                          const ChunkJob *d_job = (const ChunkJob *)d;
                          d_off = (const int32_t *)(d + b_job);
                          const ChunkGeom *d_geom = (const ChunkGeom *)(d + b_job + b_off);
                          if (mode == kChunkPlace) hipLaunchKernelGGL(zs_chunk_place_kernel, grid, block, 0, s, d_job, d_off, m, first, d_geom);
                          else if (mode == kChunkGather) hipLaunchKernelGGL(zs_chunk_gather_kernel, grid, block, 0, s, d_job, d_off, m, first, d_geom);
                          else hipLaunchKernelGGL(zs_chunk_survey_kernel, grid, block, 0, s, d_job, d_off, m, first, d_geom, d_rec);
                      }))
        return false;
    if (mode != kChunkSurvey) return true;
    hipLaunchKernelGGL(zs_chunk_fold_kernel, dim3((unsigned)((m + kChunkItemsPerWg - 1) / kChunkItemsPerWg)), dim3(64 * kChunkItemsPerWg), 0, s, d_off, m, (const uint8_t *)d_rec,
                       d_rec + n_rec);
    ZS_HIP(c, hipGetLastError());
    flags->resize((size_t)m);
    ZS_HIP(c, hipMemcpyAsync(flags->data(), d_rec + n_rec, (size_t)m, hipMemcpyDeviceToHost, s));
    ZS_HIP(c, hipStreamSynchronize(s));
    return true;
}

struct ChunkDims {
    int64_t n_chunks, chunk_bytes, array_bytes;
};
// the grids of a call: false for one that breaks a rule or whose chunk is above what one call of the engine takes
bool chunk_grids(zs_ctx *c, int n, const zs_chunk_grid *grids, std::vector<ChunkDims> *dims, int64_t *total_chunks) {
    dims->resize((size_t)n);
    *total_chunks = 0;
    for (int i = 0; i < n; i++) {
        ChunkDims &d = (*dims)[(size_t)i];
        if (!chunk_grid_check((const ChunkGrid &)grids[i], &d.n_chunks, &d.chunk_bytes, &d.array_bytes) || d.chunk_bytes > kChunkMaxBytes) {
            c->err = "stream error";
            return false;
        }
        *total_chunks += d.n_chunks;
        if (*total_chunks > 0x7FFFFFFF / 2) {
            c->err = "stream error: too many chunks in one call (split the batch)";
            return false;
        }
    }
    return true;
}

// a chunk's bytes as the kernels take them: plain where nothing was shuffled (one-byte elements: the same bytes either way)
bool chunk_plain(const zs_chunk_grid &g, int flags) { return !g.shuffle || g.elem_size == 1 || (flags & kChunkUnshuffled); }

int shuffle_call(zs_ctx *c, int n, const void *const *in, void *const *out, const int64_t *len, const int *elem_size, bool forward, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!in || !out || !len || !elem_size) return ZS_STREAM_ERROR;
    for (int i = 0; i < n; i++)
        if (len[i] < 0 || len[i] > 0x7FFFFFFF || elem_size[i] < 1 || elem_size[i] > kChunkMaxElem || (len[i] > 0 && (!in[i] || !out[i]))) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    // a buffer is a one-chunk array of one row, its leftover bytes a second one of plain bytes; the shuffled side is the chunk
    ChunkSet set;
    set.full = forward;
    auto add = [&](int64_t count, int es, const uint8_t *planes, const uint8_t *arr, int flags) {
        ChunkGrid g;
        memset(&g, 0, sizeof g);
        g.rank = 1, g.elem_size = es, g.shape[0] = g.chunk[0] = count;
        set.chunk(g, set.geom(g), 0, planes, arr, flags);
    };
    for (int i = 0; i < n; i++) {
        const int64_t count = len[i] / elem_size[i], left = len[i] % elem_size[i];
        const uint8_t *planes = (const uint8_t *)(forward ? out[i] : in[i]), *arr = (const uint8_t *)(forward ? in[i] : out[i]);
        if (count) add(count, elem_size[i], planes, arr, elem_size[i] == 1 ? kJobPlain : 0);
        if (left) add(left, 1, planes + count * elem_size[i], arr + count * elem_size[i], kJobPlain);
    }
    bool no_memory = false;
    double ms = 0;
    if (!chunk_run(c, set, forward ? kChunkGather : kChunkPlace, s, &no_memory, &ms)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    png_set_stage(c, kStChunk, ms);
    return png_done(hip_stream, s);
}
}  // namespace

extern "C" int zs_chunk_grid_info(const zs_chunk_grid *grid, int64_t *n_chunks, int64_t *chunk_bytes, int64_t *array_bytes) {
    int64_t n = 0, cb = 0, ab = 0;
    if (!grid || !chunk_grid_check(*(const ChunkGrid *)grid, &n, &cb, &ab)) return ZS_STREAM_ERROR;
    if (n_chunks) *n_chunks = n;
    if (chunk_bytes) *chunk_bytes = cb;
    if (array_bytes) *array_bytes = ab;
    return ZS_OK;
}

extern "C" int64_t zs_chunks_bound(const zs_chunk_grid *grid) {
    int64_t n = 0, cb = 0, ab = 0, r = 0;
    if (!grid || !chunk_grid_check(*(const ChunkGrid *)grid, &n, &cb, &ab)) return -1;
    const int64_t per = zs_wrap_bound(cb, grid->wrap);
    return per >= 0 && chunk_mul(n, per, &r) ? r : -1;
}

extern "C" int zs_shuffle_batch_device(zs_ctx *c, int n, const void *const *in, void *const *out, const int64_t *len, const int *elem_size, void *hip_stream) {
    return shuffle_call(c, n, in, out, len, elem_size, true, hip_stream);
}

extern "C" int zs_unshuffle_batch_device(zs_ctx *c, int n, const void *const *in, void *const *out, const int64_t *len, const int *elem_size, void *hip_stream) {
    return shuffle_call(c, n, in, out, len, elem_size, false, hip_stream);
}

extern "C" int zs_chunks_decode_batch(zs_ctx *c, int n, const zs_chunk_grid *grids, const zs_chunk_ref *const *chunks, void *const *out, const int64_t *out_cap,
                                      int *const *chunk_status, int *status, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!grids || !chunks || !out || !out_cap) return ZS_STREAM_ERROR;
    std::vector<ChunkDims> dims;
    int64_t total_chunks = 0;
    if (!chunk_grids(c, n, grids, &dims, &total_chunks)) return ZS_STREAM_ERROR;
    // ---- the chunks' places in the upload, and every chunk's route; the arrays without room are left out of everything
    struct Ref {
        int array;
        int64_t chunk;
        size_t up, buf;  // its bytes in the upload; its place in the context's buffer (a stream's)
    };
    std::vector<int> st((size_t)n, ZS_OK);
    std::vector<std::vector<int>> cst((size_t)n);
    std::vector<std::vector<std::string>> cwhy((size_t)n);
    std::vector<Ref> streams[3], stored, missing;
    size_t up_total = 0, buf_total = 0;
    int64_t items = 0;
    for (int i = 0; i < n; i++) {
        if (!chunks[i] || !out[i] || out_cap[i] < 0) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        const ChunkDims &d = dims[(size_t)i];
        const ChunkGeom geom = chunk_geom((const ChunkGrid &)grids[i]);
        const bool fits = out_cap[i] >= d.array_bytes;
        if (!fits) st[(size_t)i] = ZS_BUF_ERROR;
        else cst[(size_t)i].assign((size_t)d.n_chunks, ZS_OK), cwhy[(size_t)i].resize((size_t)d.n_chunks);
        for (int64_t k = 0; k < d.n_chunks; k++) {
            const zs_chunk_ref &r = chunks[i][k];
            if (r.len < 0 || r.len > kChunkMaxBytes || (r.flags & ~(kChunkStored | kChunkUnshuffled | kChunkSkip))) {
                c->err = "stream error";
                return ZS_STREAM_ERROR;
            }
            if (!fits || (r.flags & kChunkSkip)) continue;
            Ref ref{i, k, 0, 0};
            int32_t ext[kChunkMaxRank];
            if (!r.data) {
                missing.push_back(ref);
            } else if (r.flags & kChunkStored) {
                if (r.len != d.chunk_bytes) {
                    cst[(size_t)i][(size_t)k] = ZS_DATA_ERROR, cwhy[(size_t)i][(size_t)k] = "incorrect chunk length";
                    continue;
                }
                ref.up = up_total, up_total += ((size_t)r.len + 255) & ~(size_t)255;
                stored.push_back(ref);
            } else {
                ref.up = up_total, up_total += ((size_t)r.len + 255) & ~(size_t)255;
                ref.buf = buf_total, buf_total += ((size_t)d.chunk_bytes + 255) & ~(size_t)255;
                streams[grids[i].wrap].push_back(ref);
            }
            (void)chunk_place_of((const ChunkGrid &)grids[i], k, ext);
            items += chunk_item_count(geom, ext, false);
        }
    }
    if (!chunk_items_ok(c, items)) return ZS_STREAM_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    auto finish = [&](int rc) {
        if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
        return rc;
    };
    auto fail_all = [&](int rc) {
        std::fill(st.begin(), st.end(), rc);
        return finish(rc);
    };
    // ---- the chunks' bytes, one copy
    if (!ensure(c, c->png[kBufWrapFiles], up_total + 256) || !ensure(c, c->png[kBufChunkData], buf_total + 256) || !ensure_pinned(c, up_total + 256)) return fail_all(ZS_MEM_ERROR);
    uint8_t *d_up = (uint8_t *)c->png[kBufWrapFiles].p, *d_buf = (uint8_t *)c->png[kBufChunkData].p;
    auto stage = [&](const std::vector<Ref> &refs) {
        for (const Ref &r : refs) {
            const zs_chunk_ref &ch = chunks[r.array][r.chunk];
            if (ch.len) memcpy((uint8_t *)c->pinned + r.up, ch.data, (size_t)ch.len);
        }
    };
    stage(stored);
    for (const std::vector<Ref> &g : streams) stage(g);
    if (up_total && hipMemcpyAsync(d_up, c->pinned, up_total, hipMemcpyHostToDevice, s) != hipSuccess) return fail_all(ZS_STREAM_ERROR);
    if (hipStreamSynchronize(s) != hipSuccess) return fail_all(ZS_STREAM_ERROR);  // (the inflate call below takes the pinned buffer)
    // ---- one inflate call over all compressed chunks (one per container in use), each into exactly chunk_bytes of room
    const std::string before = c->err;
    std::vector<double> inf_ms;
    ChunkSet set;
    std::vector<int> geom_of((size_t)n, -1);
    auto place = [&](const Ref &r, const uint8_t *bytes, int flags) {
        const ChunkGrid &g = (const ChunkGrid &)grids[r.array];
        if (geom_of[(size_t)r.array] < 0) geom_of[(size_t)r.array] = set.geom(g);
        set.chunk(g, geom_of[(size_t)r.array], r.chunk, bytes, out[r.array], flags);
    };
    for (int wrap = ZS_WRAP_ZLIB; wrap <= ZS_WRAP_GZIP; wrap++) {
        const std::vector<Ref> &refs = streams[wrap];
        const int m = (int)refs.size();
        if (m == 0) continue;
        std::vector<const void *> sin((size_t)m);
        std::vector<void *> sout((size_t)m);
        std::vector<int64_t> slen((size_t)m), scap((size_t)m), olen((size_t)m, 0);
        std::vector<int> sst((size_t)m, ZS_STREAM_ERROR);
        for (int j = 0; j < m; j++) {
            const Ref &r = refs[(size_t)j];
            sin[(size_t)j] = d_up + r.up, slen[(size_t)j] = chunks[r.array][r.chunk].len;
            sout[(size_t)j] = d_buf + r.buf, scap[(size_t)j] = dims[(size_t)r.array].chunk_bytes;
        }
        (void)zs_inflate_wrap_batch_device(c, m, sin.data(), slen.data(), sout.data(), scap.data(), olen.data(), nullptr, sst.data(), wrap, (void *)s);
        if (c->profiling) inf_ms.assign(c->stage_ms, c->stage_ms + kStCount);
        bool first = true;  // the call's message is its first failing stream's
        for (int j = 0; j < m; j++) {
            const Ref &r = refs[(size_t)j];
            if (sst[(size_t)j] == ZS_STREAM_ERROR || sst[(size_t)j] == ZS_OK || sst[(size_t)j] == ZS_MEM_ERROR) return fail_all(sst[(size_t)j] == ZS_MEM_ERROR ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
            int &code = cst[(size_t)r.array][(size_t)r.chunk];
            std::string &why = cwhy[(size_t)r.array][(size_t)r.chunk];
            if (sst[(size_t)j] != ZS_STREAM_END) {
                code = sst[(size_t)j], why = first ? c->err : std::string(code == ZS_BUF_ERROR ? "buffer error" : "data error");
                first = false;
            } else if (olen[(size_t)j] != scap[(size_t)j]) {
                code = ZS_DATA_ERROR, why = "incorrect chunk length";
            } else {
                const zs_chunk_ref &ch = chunks[r.array][r.chunk];
                place(r, (const uint8_t *)sout[(size_t)j], chunk_plain(grids[r.array], ch.flags) ? kJobPlain : 0);
            }
        }
    }
    // ---- one place launch: the inflated chunks from the buffer, the stored ones from the upload, the missing ones as fill
    for (const Ref &r : stored) place(r, d_up + r.up, chunk_plain(grids[r.array], chunks[r.array][r.chunk].flags) ? kJobPlain : 0);
    for (const Ref &r : missing) place(r, nullptr, kJobFill);
    bool no_memory = false;
    double ms = 0;
    if (!chunk_run(c, set, kChunkPlace, s, &no_memory, &ms)) return fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    if (png_done(hip_stream, s) != ZS_OK) return fail_all(ZS_STREAM_ERROR);
    if (c->profiling) {
        if (inf_ms.empty()) png_set_stage(c, kStChunk, ms);
        else std::copy(inf_ms.begin(), inf_ms.end(), c->stage_ms), c->stage_ms[kStChunk] = ms;
    }
    // ---- the codes: an array's is its first failing chunk's, the call's its first failing array's
    std::vector<std::string> why((size_t)n);
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) {
            why[(size_t)i] = "buffer error";
            continue;
        }
        if (chunk_status && chunk_status[i]) memcpy(chunk_status[i], cst[(size_t)i].data(), sizeof(int) * cst[(size_t)i].size());
        for (size_t k = 0; k < cst[(size_t)i].size(); k++)
            if (cst[(size_t)i][k] != ZS_OK) {
                char head[48];
                snprintf(head, sizeof head, "chunk %lld: ", (long long)k);
                st[(size_t)i] = cst[(size_t)i][k], why[(size_t)i] = std::string(head) + cwhy[(size_t)i][k];
                break;
            }
    }
    c->err = before;
    for (int i = 0; i < n; i++)
        if (st[(size_t)i] != ZS_OK) {
            char head[48];
            snprintf(head, sizeof head, "array %d: ", i);
            c->err = std::string(head) + why[(size_t)i];
            return finish(st[(size_t)i]);
        }
    return finish(ZS_OK);
}

extern "C" int zs_chunks_encode_batch_device(zs_ctx *c, int n, const zs_chunk_grid *grids, const void *const *in, void *const *out, const int64_t *out_cap, int64_t *out_len,
                                             int64_t *const *chunk_off, int64_t *const *chunk_len, int *const *chunk_flags, int *status, int level, int strategy,
                                             int hash_variant, int options, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!grids || !in || !out || !out_cap || !out_len || !chunk_off || !chunk_len || (options & ~(ZS_CHUNKS_SKIP_FILL | ZS_CHUNKS_ALLOW_STORED))) return ZS_STREAM_ERROR;
    std::vector<ChunkDims> dims;
    int64_t total_chunks = 0;
    if (!chunk_grids(c, n, grids, &dims, &total_chunks)) return ZS_STREAM_ERROR;
    std::vector<int64_t> first((size_t)n + 1, 0);  // array i's chunks in the call's list
    int64_t items = 0;
    for (int i = 0; i < n; i++) {
        if (!in[i] || !out[i] || out_cap[i] < 0 || !chunk_off[i] || !chunk_len[i]) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        first[(size_t)i + 1] = first[(size_t)i] + dims[(size_t)i].n_chunks;
        const ChunkGeom geom = chunk_geom((const ChunkGrid &)grids[i]);
        items += dims[(size_t)i].n_chunks * chunk_item_count(geom, geom.chunk, true);  // (the gather's items; the survey has no more)
        if (!chunk_items_ok(c, items)) return ZS_STREAM_ERROR;
    }
    const int m = (int)total_chunks;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    std::vector<int> st((size_t)n, ZS_OK);
    for (int i = 0; i < n; i++) out_len[i] = 0;
    auto finish = [&](int rc) {
        if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
        return rc;
    };
    auto fail_all = [&](int rc) {
        std::fill(st.begin(), st.end(), rc);
        return finish(rc);
    };
    // chunk q of the call: its array, its number there, what becomes of it
    struct Cut {
        int array;
        int64_t chunk;
        int flags;
        size_t data, zs;  // its bytes and its stream in the context's buffers
        int64_t zlen;
    };
    std::vector<Cut> cuts((size_t)m);
    for (int i = 0; i < n; i++)
        for (int64_t k = 0; k < dims[(size_t)i].n_chunks; k++) cuts[(size_t)(first[(size_t)i] + k)] = Cut{i, k, 0, 0, 0, 0};
    bool no_memory = false;
    double ms_survey = 0, ms_gather = 0;
    std::vector<int> geom_of((size_t)n, -1);
    auto add = [&](ChunkSet &set, const Cut &t, const void *bytes, int flags) {
        const ChunkGrid &g = (const ChunkGrid &)grids[t.array];
        if (geom_of[(size_t)t.array] < 0) geom_of[(size_t)t.array] = set.geom(g);
        set.chunk(g, geom_of[(size_t)t.array], t.chunk, bytes, in[t.array], flags);
    };
    // ---- the survey: which chunks hold nothing but fill
    if (options & ZS_CHUNKS_SKIP_FILL) {
        ChunkSet set;
        for (const Cut &t : cuts) add(set, t, nullptr, 0);
        std::vector<uint8_t> same;
        if (!chunk_run(c, set, kChunkSurvey, s, &no_memory, &ms_survey, &same)) return fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
        for (size_t q = 0; q < (size_t)m; q++)
            if (same[q]) cuts[q].flags = kChunkAbsent;
        std::fill(geom_of.begin(), geom_of.end(), -1);
    }
    // ---- one gather launch: every chunk that is written, padded and shuffled, into a buffer of the context
    size_t data_total = 0, zs_total = 0;
    for (Cut &t : cuts) {
        if (t.flags & kChunkAbsent) continue;
        t.data = data_total, data_total += ((size_t)dims[(size_t)t.array].chunk_bytes + 255) & ~(size_t)255;
        t.zs = zs_total, zs_total += ((size_t)zs_wrap_bound(dims[(size_t)t.array].chunk_bytes, grids[t.array].wrap) + 255) & ~(size_t)255;
    }
    if (!ensure(c, c->png[kBufChunkData], data_total + 256) || !ensure(c, c->png[kBufChunkZs], zs_total + 256)) return fail_all(ZS_MEM_ERROR);
    uint8_t *d_data = (uint8_t *)c->png[kBufChunkData].p, *d_zs = (uint8_t *)c->png[kBufChunkZs].p;
    {
        ChunkSet set;
        set.full = true;
        for (const Cut &t : cuts)
            if (!(t.flags & kChunkAbsent)) add(set, t, d_data + t.data, chunk_plain(grids[t.array], 0) ? kJobPlain : 0);
        if (!chunk_run(c, set, kChunkGather, s, &no_memory, &ms_gather)) return fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    }
    // ---- one deflate call over all of them (one per container in use)
    for (int wrap = ZS_WRAP_ZLIB; wrap <= ZS_WRAP_GZIP; wrap++) {
        std::vector<size_t> idx;
        for (size_t q = 0; q < (size_t)m; q++)
            if (!(cuts[q].flags & kChunkAbsent) && grids[cuts[q].array].wrap == wrap) idx.push_back(q);
        const int mz = (int)idx.size();
        if (mz == 0) continue;
        std::vector<const void *> zin((size_t)mz);
        std::vector<void *> zout((size_t)mz);
        std::vector<int64_t> zin_len((size_t)mz), zcap((size_t)mz), zlen((size_t)mz, 0);
        std::vector<int> zst((size_t)mz, ZS_STREAM_ERROR);
        for (int j = 0; j < mz; j++) {
            const Cut &t = cuts[idx[(size_t)j]];
            zin[(size_t)j] = d_data + t.data, zin_len[(size_t)j] = dims[(size_t)t.array].chunk_bytes;
            zout[(size_t)j] = d_zs + t.zs, zcap[(size_t)j] = zs_wrap_bound(zin_len[(size_t)j], wrap);
        }
        const int zrc = zs_deflate_wrap_batch_device(c, mz, zin.data(), zin_len.data(), zout.data(), zcap.data(), zlen.data(), zst.data(), level, strategy, hash_variant, wrap, (void *)s);
        if (zrc != ZS_OK) return fail_all(zrc);
        for (int j = 0; j < mz; j++) cuts[idx[(size_t)j]].zlen = zlen[(size_t)j];
    }
    if (c->profiling) c->stage_ms[kStChunk] = ms_survey + ms_gather;
    // ---- the layout on the host, from the lengths the deflate call returned; which arrays fit
    int rc = ZS_OK, n_spans = 0;
    for (int i = 0; i < n; i++) {
        int64_t at = 0;
        for (int64_t k = 0; k < dims[(size_t)i].n_chunks; k++) {
            Cut &t = cuts[(size_t)(first[(size_t)i] + k)];
            int64_t len = 0;
            if (!(t.flags & kChunkAbsent)) {
                len = t.zlen;
                if ((options & ZS_CHUNKS_ALLOW_STORED) && t.zlen >= dims[(size_t)i].chunk_bytes) t.flags |= kChunkStored, len = dims[(size_t)i].chunk_bytes;
            }
            chunk_off[i][k] = at, chunk_len[i][k] = len, at += len;
            if (chunk_flags && chunk_flags[i]) chunk_flags[i][k] = t.flags;
        }
        out_len[i] = at;
        if (out_cap[i] < at) {
            st[(size_t)i] = ZS_BUF_ERROR;
            if (rc == ZS_OK) rc = ZS_BUF_ERROR, c->err = "buffer error";
        } else {
            for (int64_t k = 0; k < dims[(size_t)i].n_chunks; k++) n_spans += chunk_len[i][k] > 0;
        }
    }
    if (n_spans == 0) return finish(rc);
    // ---- one KC job: every chunk of an array that fits copied into its place
    Crc32Job job;
    if (!crc32_begin(c, n_spans, 0, &job, &no_memory)) {
        for (int i = 0; i < n; i++)
            if (st[(size_t)i] == ZS_OK) st[(size_t)i] = no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
        return finish(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    }
    int sp = 0;
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        for (int64_t k = 0; k < dims[(size_t)i].n_chunks; k++) {
            const Cut &t = cuts[(size_t)(first[(size_t)i] + k)];
            if (chunk_len[i][k] == 0) continue;
            const uint8_t *src = (t.flags & kChunkStored) ? d_data + t.data : d_zs + t.zs;
            job.spans[sp++] = Crc32Span{src, (uint8_t *)out[i] + chunk_off[i][k], nullptr, chunk_len[i][k], 0xFFFFFFFFu, 0, 0, 0};
        }
    }
    if (!crc32_run(c, &job, s)) {
        for (int i = 0; i < n; i++)
            if (st[(size_t)i] == ZS_OK) st[(size_t)i] = ZS_STREAM_ERROR;
        return finish(ZS_STREAM_ERROR);
    }
    if (c->profiling) c->stage_ms[kStCrc32] = job.ms;
    return finish(rc);
}
