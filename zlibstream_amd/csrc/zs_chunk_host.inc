// zs_chunk_host.inc -- host side of the chunked-array calls of include/zsgpu.h: the chunks of HDF5 / NetCDF-4 datasets and
// Zarr v2 arrays (shuffle in front of deflate) from host memory decoded on the device into arrays, arrays that lie there
// written as chunks, and the shuffle filter alone.  Part of zs_engine.hip's translation unit, behind zs_parts_host.inc, whose gate,
// staging and roll-up of the codes it takes (zs_parts.h), and zs_wrap_host.inc, whose container calls it calls; the
// flat-list runner (png_run_list) and the KC job runner (Crc32Job) are zs_png_host.inc's; the geometry is zs_chunk.h's, the kernels (KN) zs_chunk.hip's.  The two array calls take a zs_chunk_filters per array
// (Fletcher-32, delta, big-endian elements; null: none, the calls without filters); KL and KI are zs_chunk.hip's too, and the
// checksum and the delta filter are calls of their own as well.

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
    const size_t n_rec = pad256((size_t)set.items.total);
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

static_assert(sizeof(zs_chunk_filters) == sizeof(ChunkFilters) && offsetof(zs_chunk_filters, fletcher32) == offsetof(ChunkFilters, fletcher32), "zs_chunk_filters mirrors ChunkFilters");
static_assert(sizeof(FletSpan) % 8 == 0 && sizeof(DeltaJob) % 8 == 0 && sizeof(FletSum) == 16, "the descriptors lie in front of the tile list");
static_assert(ZS_FLETCHER32_TILE == kFletTile && ZS_DELTA_TILE == kDeltaTile, "the tiles are zs_chunk.h's");

bool chunk_tiles_ok(zs_ctx *c, int64_t total) {
    if (total <= 0x7FFFFFFF) return true;
    c->err = "stream error: more than 2^31 - 1 tiles in one call (split the batch)";
    return false;
}

// KL over the spans on `s`: the tile launch, the fold, the checksums into sums[] (two waits: the upload, the results).  A span
// with a dst has its checksum written there as well.
bool fletcher_run(zs_ctx *c, const std::vector<FletSpan> &spans, hipStream_t s, bool *no_memory, double *ms, uint32_t *sums) {
    *no_memory = false;
    const int m = (int)spans.size();
    if (m == 0) return true;
    PngOffsets tiles;
    for (const FletSpan &sp : spans) tiles.add(fletcher_tiles(sp.len));
    if (!chunk_tiles_ok(c, tiles.total)) return false;
    const size_t b_rec = sizeof(FletSum) * (size_t)tiles.total;
    if (!ensure(c, c->png[kBufChunkAux], b_rec + sizeof(uint32_t) * (size_t)m + 256)) {
        *no_memory = true;
        return false;
    }
    FletSum *d_rec = (FletSum *)c->png[kBufChunkAux].p;
    uint32_t *d_sum = (uint32_t *)((uint8_t *)c->png[kBufChunkAux].p + b_rec);
    const size_t b_sp = sizeof(FletSpan) * (size_t)m;
    const FletSpan *d_sp = (const FletSpan *)nullptr;
    const int32_t *d_off = nullptr;
    // (a call without tiles -- every span empty -- still uploads the spans: the fold reads their lengths)
    if (!png_run_list(c, c->png[kBufChunkDesc], {{spans.data(), b_sp}}, tiles, 0, kChunkGrid, s, no_memory, ms, [&](dim3 grid, dim3 block, uint8_t *d, int64_t first) {
            hipLaunchKernelGGL(zs_fletcher_tile_kernel, grid, block, 0, s, (const FletSpan *)d, (const int32_t *)(d + b_sp), m, first, d_rec);
        }))
        return false;
    d_sp = (const FletSpan *)c->png[kBufChunkDesc].p, d_off = (const int32_t *)((const uint8_t *)c->png[kBufChunkDesc].p + b_sp);
    hipLaunchKernelGGL(zs_fletcher_fold_kernel, dim3((unsigned)((m + kChunkItemsPerWg - 1) / kChunkItemsPerWg)), dim3(64 * kChunkItemsPerWg), 0, s, d_sp, d_off, m,
                       (const FletSum *)d_rec, d_sum);
    ZS_HIP(c, hipGetLastError());
    if (!ensure_pinned(c, sizeof(uint32_t) * (size_t)m)) {
        *no_memory = true;
        return false;
    }
    ZS_HIP(c, hipMemcpyAsync(c->pinned, d_sum, sizeof(uint32_t) * (size_t)m, hipMemcpyDeviceToHost, s));
    ZS_HIP(c, hipStreamSynchronize(s));
    memcpy(sums, c->pinned, sizeof(uint32_t) * (size_t)m);
    return true;
}

// KI over the jobs on `s`, left in flight (one wait, for the upload): encode in one launch, decode in three
bool delta_run(zs_ctx *c, const std::vector<DeltaJob> &jobs, bool decode, hipStream_t s, bool *no_memory, double *ms) {
    *no_memory = false;
    const int m = (int)jobs.size();
    if (m == 0) return true;
    PngOffsets tiles;
    for (const DeltaJob &jb : jobs) tiles.add(delta_tiles(jb.E, jb.left));
    if (!chunk_tiles_ok(c, tiles.total)) return false;
    if (decode && !ensure(c, c->png[kBufChunkAux], sizeof(uint64_t) * (size_t)tiles.total + 256)) {
        *no_memory = true;
        return false;
    }
    uint64_t *d_sums = (uint64_t *)c->png[kBufChunkAux].p;
    const size_t b_job = sizeof(DeltaJob) * (size_t)m;
    struct Slice {
        dim3 grid, block;
        int64_t first;
    };
    std::vector<Slice> slices;  // (the second pass goes over the same slices behind the scan)
    if (!png_run_list(c, c->png[kBufChunkDesc], {{jobs.data(), b_job}}, tiles, 0, kChunkGrid, s, no_memory, ms, [&](dim3 grid, dim3 block, uint8_t *d, int64_t first) {
            if (decode) hipLaunchKernelGGL(zs_delta_sum_kernel, grid, block, 0, s, (const DeltaJob *)d, (const int32_t *)(d + b_job), m, first, d_sums);
            else hipLaunchKernelGGL(zs_delta_encode_kernel, grid, block, 0, s, (const DeltaJob *)d, (const int32_t *)(d + b_job), m, first);
            slices.push_back(Slice{grid, block, first});
        }))
        return false;
    if (!decode) return true;
    const DeltaJob *d_job = (const DeltaJob *)c->png[kBufChunkDesc].p;
    const int32_t *d_off = (const int32_t *)((const uint8_t *)c->png[kBufChunkDesc].p + b_job);
    const bool timed = ms && c->profiling;  // (the sums' time is in *ms; the scan's and the second pass's is added)
    if (timed) (void)hipEventRecord(c->ev_png[0], s);
    hipLaunchKernelGGL(zs_delta_scan_kernel, dim3((unsigned)((m + kChunkItemsPerWg - 1) / kChunkItemsPerWg)), dim3(64 * kChunkItemsPerWg), 0, s, d_off, m, d_sums);
    ZS_HIP(c, hipGetLastError());
    for (const Slice &sl : slices) {
        hipLaunchKernelGGL(zs_delta_decode_kernel, sl.grid, sl.block, 0, s, d_job, d_off, m, sl.first, (const uint64_t *)d_sums);
        ZS_HIP(c, hipGetLastError());
    }
    if (timed) {
        (void)hipEventRecord(c->ev_png[1], s);
        ZS_HIP(c, hipStreamSynchronize(s));
        float t = 0;
        (void)hipEventElapsedTime(&t, c->ev_png[0], c->ev_png[1]);
        *ms += t;
    }
    return true;
}

struct ChunkDims {
    int64_t n_chunks, chunk_bytes, array_bytes;
};
// the grids of a call: false for one that breaks a rule or whose chunk is above what one call of the engine takes
// (filters may be null: none)
bool chunk_grids(zs_ctx *c, int n, const zs_chunk_grid *grids, const zs_chunk_filters *filters, std::vector<ChunkDims> *dims, int64_t *total_chunks) {
    dims->resize((size_t)n);
    *total_chunks = 0;
    for (int i = 0; i < n; i++) {
        ChunkDims &d = (*dims)[(size_t)i];
        if (!chunk_grid_check((const ChunkGrid &)grids[i], &d.n_chunks, &d.chunk_bytes, &d.array_bytes) || d.chunk_bytes > kChunkMaxBytes ||
            (filters && !chunk_filters_check(grids[i].elem_size, (const ChunkFilters &)filters[i]))) {
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

namespace {
// zs_chunks_decode_filters_batch; filters null: zs_chunks_decode_batch
int chunks_decode(zs_ctx *c, int n, const zs_chunk_grid *grids, const zs_chunk_filters *filters, const zs_chunk_ref *const *chunks, void *const *out, const int64_t *out_cap,
                  int *const *chunk_status, int *status, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!grids || !chunks || !out || !out_cap) return ZS_STREAM_ERROR;
    std::vector<ChunkDims> dims;
    int64_t total_chunks = 0;
    if (!chunk_grids(c, n, grids, filters, &dims, &total_chunks)) return ZS_STREAM_ERROR;
    const ChunkFilters none{0, 0, 0, 0};
    auto filt = [&](int i) -> const ChunkFilters & { return filters ? (const ChunkFilters &)filters[i] : none; };
    // ---- the chunks' places in the upload, and every chunk's route; the arrays without room are left out of everything
    struct Ref {
        int array;
        int64_t chunk;
        size_t up, buf;  // its bytes in the upload; its place in the context's buffer (a stream's)
        int64_t len;     // its bytes without the checksum
    };
    CallGate gate(n, status);
    PartCodes pc(gate.st);
    std::vector<Ref> streams[3], stored, missing;
    StageLayout up(kChunkMaxBytes);  // the chunks that are uploaded, in the walk's order ...
    std::vector<const void *> up_ptr;  // ... and their bytes
    std::vector<int64_t> up_len;
    auto upload = [&](const zs_chunk_ref &r) {
        up_ptr.push_back(r.data), up_len.push_back(r.len);
        return up.add(r.len);
    };
    size_t buf_total = 0;
    int64_t items = 0;
    for (int i = 0; i < n; i++) {
        if (!chunks[i] || !out[i] || out_cap[i] < 0) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        const ChunkDims &d = dims[(size_t)i];
        const ChunkGeom geom = chunk_geom((const ChunkGrid &)grids[i]);
        const bool fits = out_cap[i] >= d.array_bytes;
        if (!fits) pc.fail_file(i, ZS_BUF_ERROR, "buffer error");
        else pc.open_parts(i, (size_t)d.n_chunks);
        for (int64_t k = 0; k < d.n_chunks; k++) {
            const zs_chunk_ref &r = chunks[i][k];
            if (r.len < 0 || r.len > kChunkMaxBytes || (r.flags & ~(kChunkStored | kChunkUnshuffled | kChunkSkip))) {
                c->err = "stream error";
                return ZS_STREAM_ERROR;
            }
            if (!fits || (r.flags & kChunkSkip)) continue;
            const int tail = filt(i).fletcher32 ? 4 : 0;  // the checksum behind the chunk's bytes
            Ref ref{i, k, 0, 0, r.len - tail};
            int32_t ext[kChunkMaxRank];
            if (!r.data) {
                missing.push_back(ref);
            } else if (r.len < tail || ((r.flags & kChunkStored) && ref.len != d.chunk_bytes)) {
                pc.fail_part(i, k, ZS_DATA_ERROR, "incorrect chunk length");
                continue;
            } else if (r.flags & kChunkStored) {
                ref.up = upload(r);
                stored.push_back(ref);
            } else {
                ref.up = upload(r);
                ref.buf = buf_total, buf_total += pad256((size_t)d.chunk_bytes);
                streams[grids[i].wrap].push_back(ref);
            }
            (void)chunk_place_of((const ChunkGrid &)grids[i], k, ext);
            items += chunk_item_count(geom, ext, false);
        }
    }
    if (!chunk_items_ok(c, items)) return ZS_STREAM_ERROR;
    if (!gate.open(c, hip_stream, nullptr)) return ZS_STREAM_ERROR;
    hipStream_t s = gate.s;
    // ---- the chunks' bytes, one copy
    if (!ensure(c, c->png[kBufChunkData], buf_total + 256)) return gate.fail_all(ZS_MEM_ERROR);
    uint8_t *d_up = nullptr, *d_buf = (uint8_t *)c->png[kBufChunkData].p;
    if (const int rc = stage_files(c, up, up_ptr.data(), up_len.data(), s, &d_up)) return gate.fail_all(rc);
    // ---- Fletcher-32: one KL job over every chunk that carries one, as it lies behind the upload; the host compares with the
    // four bytes it holds, and a chunk that differs goes no further
    bool no_memory = false;
    double ms_filters = 0, ms_part = 0;
    {
        std::vector<FletSpan> spans;
        std::vector<std::vector<Ref> *> lists{&stored, &streams[0], &streams[1], &streams[2]};
        for (std::vector<Ref> *l : lists)
            for (const Ref &r : *l)
                if (filt(r.array).fletcher32) spans.push_back(FletSpan{d_up + r.up, nullptr, r.len});
        if (!spans.empty()) {
            std::vector<uint32_t> sums(spans.size());
            if (!fletcher_run(c, spans, s, &no_memory, &ms_part, sums.data())) return gate.fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
            ms_filters += ms_part;
            size_t q = 0;
            for (std::vector<Ref> *l : lists) {
                std::vector<Ref> keep;
                for (const Ref &r : *l) {
                    if (filt(r.array).fletcher32) {
                        const uint8_t *t = (const uint8_t *)chunks[r.array][r.chunk].data + r.len;
                        const uint32_t want = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
                        if (sums[q++] != want) {
                            pc.fail_part(r.array, r.chunk, ZS_DATA_ERROR, "incorrect chunk checksum");
                            continue;
                        }
                    }
                    keep.push_back(r);
                }
                l->swap(keep);
            }
        }
    }
    // ---- one inflate call over all compressed chunks (one per container in use), each into exactly chunk_bytes of room
    const std::string before = c->err;
    std::string first_err[3];  // per container: the message of the inflate call's first failing stream
    std::vector<double> inf_ms;
    ChunkSet set;
    std::vector<int> geom_of((size_t)n, -1);
    struct Whole {
        Ref r;
        const uint8_t *bytes;
        int flags;
    };
    std::vector<Whole> whole;  // the chunks that are placed: with delta through KI first, whose places come behind this list
    auto place = [&](const Ref &r, const uint8_t *bytes, int flags) { whole.push_back(Whole{r, bytes, flags}); };
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
            sin[(size_t)j] = d_up + r.up, slen[(size_t)j] = r.len;
            sout[(size_t)j] = d_buf + r.buf, scap[(size_t)j] = dims[(size_t)r.array].chunk_bytes;
        }
        (void)zs_inflate_wrap_batch_device(c, m, sin.data(), slen.data(), sout.data(), scap.data(), olen.data(), nullptr, sst.data(), wrap, (void *)s);
        if (c->profiling) inf_ms.assign(c->stage_ms, c->stage_ms + kStCount);
        bool first = true;  // the call's message is its first failing stream's
        for (int j = 0; j < m; j++) {
            const Ref &r = refs[(size_t)j];
            // (zs_inflate_wrap_batch_device, unlike run_inflate under inflate_parts, reports a call that ran out of memory per stream)
            if (sst[(size_t)j] == ZS_STREAM_ERROR || sst[(size_t)j] == ZS_OK || sst[(size_t)j] == ZS_MEM_ERROR) return gate.fail_all(sst[(size_t)j] == ZS_MEM_ERROR ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
            if (sst[(size_t)j] != ZS_STREAM_END) {
                if (first) first_err[wrap] = c->err;
                pc.fail_part(r.array, r.chunk, sst[(size_t)j], first ? first_err[wrap].c_str() : sst[(size_t)j] == ZS_BUF_ERROR ? "buffer error" : "data error");
                first = false;
            } else if (olen[(size_t)j] != scap[(size_t)j]) {
                pc.fail_part(r.array, r.chunk, ZS_DATA_ERROR, "incorrect chunk length");
            } else {
                const zs_chunk_ref &ch = chunks[r.array][r.chunk];
                place(r, (const uint8_t *)sout[(size_t)j], chunk_plain(grids[r.array], ch.flags) ? kJobPlain : 0);
            }
        }
    }
    // ---- one place launch: the inflated chunks from the buffer, the stored ones from the upload, the missing ones as fill
    for (const Ref &r : stored) place(r, d_up + r.up, chunk_plain(grids[r.array], chunks[r.array][r.chunk].flags) ? kJobPlain : 0);
    for (const Ref &r : missing) place(r, nullptr, kJobFill);
    // ---- delta: one KI job undoes it for every chunk that has it, unshuffling and reversing as it reads, into a third buffer
    // of plain little-endian elements
    {
        size_t delta_total = 0;
        for (const Whole &w : whole)
            if (filt(w.r.array).delta && !(w.flags & kJobFill)) delta_total += pad256((size_t)dims[(size_t)w.r.array].chunk_bytes);
        if (delta_total && !ensure(c, c->png[kBufChunkDelta], delta_total + 256)) return gate.fail_all(ZS_MEM_ERROR);
        uint8_t *d_delta = (uint8_t *)c->png[kBufChunkDelta].p;
        std::vector<DeltaJob> jobs;
        size_t at = 0;
        for (Whole &w : whole) {
            const zs_chunk_grid &g = grids[w.r.array];
            const bool swap = filt(w.r.array).byte_order && g.elem_size > 1;
            if (w.flags & kJobFill) continue;
            if (!filt(w.r.array).delta) {
                w.flags |= swap ? kJobSwap : 0;
                continue;
            }
            const int64_t cb = dims[(size_t)w.r.array].chunk_bytes;
            jobs.push_back(DeltaJob{w.bytes, d_delta + at, cb / g.elem_size, g.elem_size, ((w.flags & kJobPlain) ? 0 : kDeltaShuffled) | (swap ? kDeltaSwap : 0), 0, 0});
            w.bytes = d_delta + at, w.flags = kJobPlain, at += pad256((size_t)cb);
        }
        ms_part = 0;
        if (!delta_run(c, jobs, true, s, &no_memory, &ms_part)) return gate.fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
        ms_filters += ms_part;
    }
    for (const Whole &w : whole) {
        const ChunkGrid &g = (const ChunkGrid &)grids[w.r.array];
        if (geom_of[(size_t)w.r.array] < 0) geom_of[(size_t)w.r.array] = set.geom(g);
        set.chunk(g, geom_of[(size_t)w.r.array], w.r.chunk, w.bytes, out[w.r.array], w.flags);
    }
    double ms = 0;
    if (!chunk_run(c, set, kChunkPlace, s, &no_memory, &ms)) return gate.fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    ms += ms_filters;
    if (png_done(hip_stream, s) != ZS_OK) return gate.fail_all(ZS_STREAM_ERROR);
    if (c->profiling) {
        if (inf_ms.empty()) png_set_stage(c, kStChunk, ms);
        else std::copy(inf_ms.begin(), inf_ms.end(), c->stage_ms), c->stage_ms[kStChunk] = ms;
    }
    return gate.finish(pc.roll_up("array", "chunk", chunk_status, before, &c->err));
}

// zs_chunks_encode_filters_batch_device; filters null: zs_chunks_encode_batch_device
int chunks_encode(zs_ctx *c, int n, const zs_chunk_grid *grids, const zs_chunk_filters *filters, const void *const *in, void *const *out, const int64_t *out_cap, int64_t *out_len,
                  int64_t *const *chunk_off, int64_t *const *chunk_len, int *const *chunk_flags, int *status, int level, int strategy, int hash_variant, int options,
                  void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!grids || !in || !out || !out_cap || !out_len || !chunk_off || !chunk_len || (options & ~(ZS_CHUNKS_SKIP_FILL | ZS_CHUNKS_ALLOW_STORED))) return ZS_STREAM_ERROR;
    std::vector<ChunkDims> dims;
    int64_t total_chunks = 0;
    if (!chunk_grids(c, n, grids, filters, &dims, &total_chunks)) return ZS_STREAM_ERROR;
    const ChunkFilters none{0, 0, 0, 0};
    auto filt = [&](int i) -> const ChunkFilters & { return filters ? (const ChunkFilters &)filters[i] : none; };
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
    CallGate gate(n, status);
    if (!gate.open(c, hip_stream, out_len)) return ZS_STREAM_ERROR;
    hipStream_t s = gate.s;
    std::vector<int> &st = gate.st;
    // chunk q of the call: its array, its number there, what becomes of it
    struct Cut {
        int array;
        int64_t chunk;
        int flags;
        size_t data, zs;  // its bytes and its stream in the context's buffers
        int64_t zlen;
        const uint8_t *src;  // its bytes as they are deflated or stored: in the gather's buffer, or behind KI in the delta buffer
    };
    std::vector<Cut> cuts((size_t)m);
    for (int i = 0; i < n; i++)
        for (int64_t k = 0; k < dims[(size_t)i].n_chunks; k++) cuts[(size_t)(first[(size_t)i] + k)] = Cut{i, k, 0, 0, 0, 0, nullptr};
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
        if (!chunk_run(c, set, kChunkSurvey, s, &no_memory, &ms_survey, &same)) return gate.fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
        for (size_t q = 0; q < (size_t)m; q++)
            if (same[q]) cuts[q].flags = kChunkAbsent;
        std::fill(geom_of.begin(), geom_of.end(), -1);
    }
    // ---- one gather launch: every chunk that is written, padded and shuffled, into a buffer of the context
    size_t data_total = 0, zs_total = 0;
    for (Cut &t : cuts) {
        if (t.flags & kChunkAbsent) continue;
        t.data = data_total, data_total += pad256((size_t)dims[(size_t)t.array].chunk_bytes);
        t.zs = zs_total, zs_total += pad256((size_t)zs_wrap_bound(dims[(size_t)t.array].chunk_bytes, grids[t.array].wrap));
    }
    if (!ensure(c, c->png[kBufChunkData], data_total + 256) || !ensure(c, c->png[kBufChunkZs], zs_total + 256)) return gate.fail_all(ZS_MEM_ERROR);
    uint8_t *d_data = (uint8_t *)c->png[kBufChunkData].p, *d_zs = (uint8_t *)c->png[kBufChunkZs].p;
    {
        // (a chunk with delta is gathered plain and little-endian: KI writes the byte order and the planes)
        ChunkSet set;
        set.full = true;
        size_t delta_total = 0;
        for (Cut &t : cuts) {
            if (t.flags & kChunkAbsent) continue;
            const bool swap = filt(t.array).byte_order && grids[t.array].elem_size > 1;
            t.src = d_data + t.data;
            if (filt(t.array).delta) add(set, t, d_data + t.data, kJobPlain), delta_total += pad256((size_t)dims[(size_t)t.array].chunk_bytes);
            else add(set, t, d_data + t.data, (chunk_plain(grids[t.array], 0) ? kJobPlain : 0) | (swap ? kJobSwap : 0));
        }
        if (!chunk_run(c, set, kChunkGather, s, &no_memory, &ms_gather)) return gate.fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
        if (delta_total) {
            if (!ensure(c, c->png[kBufChunkDelta], delta_total + 256)) return gate.fail_all(ZS_MEM_ERROR);
            uint8_t *d_delta = (uint8_t *)c->png[kBufChunkDelta].p;
            std::vector<DeltaJob> jobs;
            size_t at = 0;
            for (Cut &t : cuts) {
                if ((t.flags & kChunkAbsent) || !filt(t.array).delta) continue;
                const zs_chunk_grid &g = grids[t.array];
                const int64_t cb = dims[(size_t)t.array].chunk_bytes;
                const bool swap = filt(t.array).byte_order && g.elem_size > 1;
                jobs.push_back(DeltaJob{t.src, d_delta + at, cb / g.elem_size, g.elem_size, (chunk_plain(g, 0) ? 0 : kDeltaShuffled) | (swap ? kDeltaSwap : 0), 0, 0});
                t.src = d_delta + at, at += pad256((size_t)cb);
            }
            double ms_delta = 0;
            if (!delta_run(c, jobs, false, s, &no_memory, &ms_delta)) return gate.fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
            ms_gather += ms_delta;
        }
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
            zin[(size_t)j] = t.src, zin_len[(size_t)j] = dims[(size_t)t.array].chunk_bytes;
            zout[(size_t)j] = d_zs + t.zs, zcap[(size_t)j] = zs_wrap_bound(zin_len[(size_t)j], wrap);
        }
        const int zrc = zs_deflate_wrap_batch_device(c, mz, zin.data(), zin_len.data(), zout.data(), zcap.data(), zlen.data(), zst.data(), level, strategy, hash_variant, wrap, (void *)s);
        if (zrc != ZS_OK) return gate.fail_all(zrc);
        for (int j = 0; j < mz; j++) cuts[idx[(size_t)j]].zlen = zlen[(size_t)j];
    }
    if (c->profiling) c->stage_ms[kStChunk] = ms_survey + ms_gather;
    // ---- the layout on the host, from the lengths the deflate call returned; which arrays fit
    int rc = ZS_OK, n_spans = 0;
    for (int i = 0; i < n; i++) {
        int64_t at = 0;
        const int tail = filt(i).fletcher32 ? 4 : 0;  // the checksum behind every chunk that is written
        for (int64_t k = 0; k < dims[(size_t)i].n_chunks; k++) {
            Cut &t = cuts[(size_t)(first[(size_t)i] + k)];
            int64_t len = 0;
            if (!(t.flags & kChunkAbsent)) {
                len = t.zlen;
                if ((options & ZS_CHUNKS_ALLOW_STORED) && t.zlen >= dims[(size_t)i].chunk_bytes) t.flags |= kChunkStored, len = dims[(size_t)i].chunk_bytes;
                len += tail;
            }
            chunk_off[i][k] = at, chunk_len[i][k] = len, at += len;
            if (chunk_flags && chunk_flags[i]) chunk_flags[i][k] = t.flags;
        }
        out_len[i] = at;
    }
    (void)mark_fit(st, out_len, out_cap, &rc, &c->err);
    for (int i = 0; i < n; i++)
        if (st[(size_t)i] == ZS_OK)
            for (int64_t k = 0; k < dims[(size_t)i].n_chunks; k++) n_spans += chunk_len[i][k] > 0;
    if (n_spans == 0) return gate.finish(rc);
    // ---- one KC job: every chunk of an array that fits copied into its place
    Crc32Job job;
    if (!crc32_begin(c, n_spans, 0, &job, &no_memory)) return gate.fail_live(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    int sp = 0;
    std::vector<FletSpan> sums;  // the placed chunks that get a checksum behind them
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        const int tail = filt(i).fletcher32 ? 4 : 0;
        for (int64_t k = 0; k < dims[(size_t)i].n_chunks; k++) {
            const Cut &t = cuts[(size_t)(first[(size_t)i] + k)];
            if (chunk_len[i][k] == 0) continue;
            const uint8_t *src = (t.flags & kChunkStored) ? t.src : d_zs + t.zs;
            uint8_t *dst = (uint8_t *)out[i] + chunk_off[i][k];
            job.spans[sp++] = Crc32Span{src, dst, nullptr, chunk_len[i][k] - tail, 0xFFFFFFFFu, 0, 0, 0};
            if (tail) sums.push_back(FletSpan{dst, dst + chunk_len[i][k] - tail, chunk_len[i][k] - tail});
        }
    }
    if (!crc32_run(c, &job, s)) return gate.fail_live(ZS_STREAM_ERROR);
    if (c->profiling) c->stage_ms[kStCrc32] = job.ms;
    // ---- Fletcher-32: one KL job over the placed chunks, whose fold writes the four bytes behind each
    if (!sums.empty()) {
        std::vector<uint32_t> got(sums.size());
        double ms_sum = 0;
        if (!fletcher_run(c, sums, s, &no_memory, &ms_sum, got.data())) return gate.fail_live(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
        if (c->profiling) c->stage_ms[kStChunk] += ms_sum;
    }
    return gate.finish(rc);
}
}  // namespace

extern "C" int zs_chunks_decode_batch(zs_ctx *c, int n, const zs_chunk_grid *grids, const zs_chunk_ref *const *chunks, void *const *out, const int64_t *out_cap,
                                      int *const *chunk_status, int *status, void *hip_stream) {
    return chunks_decode(c, n, grids, nullptr, chunks, out, out_cap, chunk_status, status, hip_stream);
}

extern "C" int zs_chunks_decode_filters_batch(zs_ctx *c, int n, const zs_chunk_grid *grids, const zs_chunk_filters *filters, const zs_chunk_ref *const *chunks, void *const *out,
                                              const int64_t *out_cap, int *const *chunk_status, int *status, void *hip_stream) {
    if (n > 0 && !filters) return ZS_STREAM_ERROR;
    return chunks_decode(c, n, grids, filters, chunks, out, out_cap, chunk_status, status, hip_stream);
}

extern "C" int zs_chunks_encode_batch_device(zs_ctx *c, int n, const zs_chunk_grid *grids, const void *const *in, void *const *out, const int64_t *out_cap, int64_t *out_len,
                                             int64_t *const *chunk_off, int64_t *const *chunk_len, int *const *chunk_flags, int *status, int level, int strategy,
                                             int hash_variant, int options, void *hip_stream) {
    return chunks_encode(c, n, grids, nullptr, in, out, out_cap, out_len, chunk_off, chunk_len, chunk_flags, status, level, strategy, hash_variant, options, hip_stream);
}

extern "C" int zs_chunks_encode_filters_batch_device(zs_ctx *c, int n, const zs_chunk_grid *grids, const zs_chunk_filters *filters, const void *const *in, void *const *out,
                                                     const int64_t *out_cap, int64_t *out_len, int64_t *const *chunk_off, int64_t *const *chunk_len, int *const *chunk_flags,
                                                     int *status, int level, int strategy, int hash_variant, int options, void *hip_stream) {
    if (n > 0 && !filters) return ZS_STREAM_ERROR;
    return chunks_encode(c, n, grids, filters, in, out, out_cap, out_len, chunk_off, chunk_len, chunk_flags, status, level, strategy, hash_variant, options, hip_stream);
}

extern "C" int64_t zs_chunks_filters_bound(const zs_chunk_grid *grid, const zs_chunk_filters *filters) {
    int64_t n = 0, cb = 0, ab = 0, extra = 0, r = 0;
    if (!grid || !filters || !chunk_grid_check(*(const ChunkGrid *)grid, &n, &cb, &ab) || !chunk_filters_check(grid->elem_size, *(const ChunkFilters *)filters)) return -1;
    const int64_t base = zs_chunks_bound(grid);
    if (base < 0 || !chunk_mul(n, filters->fletcher32 ? 4 : 0, &extra) || __builtin_add_overflow(base, extra, &r)) return -1;
    return r;
}

extern "C" int zs_fletcher32_batch_device(zs_ctx *c, int n, const void *const *in, const int64_t *len, uint32_t *out, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!in || !len || !out) return ZS_STREAM_ERROR;
    std::vector<FletSpan> spans((size_t)n);
    for (int i = 0; i < n; i++) {
        if (len[i] < 0 || len[i] > 0x7FFFFFFF || (len[i] > 0 && !in[i])) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        spans[(size_t)i] = FletSpan{(const uint8_t *)in[i], nullptr, len[i]};
    }
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    bool no_memory = false;
    double ms = 0;
    if (!fletcher_run(c, spans, s, &no_memory, &ms, out)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    png_set_stage(c, kStChunk, ms);
    return ZS_OK;
}

namespace {
int delta_call(zs_ctx *c, int n, const void *const *in, void *const *out, const int64_t *len, const int *elem_size, bool decode, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!in || !out || !len || !elem_size) return ZS_STREAM_ERROR;
    std::vector<DeltaJob> jobs((size_t)n);
    for (int i = 0; i < n; i++) {
        const int es = elem_size[i];
        if (len[i] < 0 || len[i] > 0x7FFFFFFF || !(es == 1 || es == 2 || es == 4 || es == 8) || (len[i] > 0 && (!in[i] || !out[i]))) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        jobs[(size_t)i] = DeltaJob{(const uint8_t *)in[i], (uint8_t *)out[i], len[i] / es, es, 0, (int32_t)(len[i] % es), 0};
    }
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    bool no_memory = false;
    double ms = 0;
    if (!delta_run(c, jobs, decode, s, &no_memory, &ms)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    png_set_stage(c, kStChunk, ms);
    return png_done(hip_stream, s);
}
}  // namespace

extern "C" int zs_delta_encode_batch_device(zs_ctx *c, int n, const void *const *in, void *const *out, const int64_t *len, const int *elem_size, void *hip_stream) {
    return delta_call(c, n, in, out, len, elem_size, false, hip_stream);
}

extern "C" int zs_delta_decode_batch_device(zs_ctx *c, int n, const void *const *in, void *const *out, const int64_t *len, const int *elem_size, void *hip_stream) {
    return delta_call(c, n, in, out, len, elem_size, true, hip_stream);
}
