// zs_exr_host.inc -- host side of the OpenEXR calls of include/zsgpu.h: whole ZIP / ZIPS files from host memory decoded on the
// device into channel planes, and files written on the device from planes that lie there.  Part of zs_engine.hip's translation
// unit, behind zs_parts_host.inc and zs_tiff_host.inc: the call's gate, the staging, the zlib header's rules, the raw inflate of
// sub-streams, the Adler-32 compare, the roll-up of the codes and the one deflate call are zs_parts.h's and
// zs_parts_host.inc's, the flat-list runner (png_run_list) and the KC job runner (Crc32Job) zs_png_host.inc's; the
// container's rules are zs_exr.h's, the predictor kernels (KE) zs_exr.hip's.

namespace {
static_assert(sizeof(zs_exr_info) == sizeof(ExrInfo) && offsetof(zs_exr_info, out_len) == offsetof(ExrInfo, out_len) && offsetof(zs_exr_info, tiled) == offsetof(ExrInfo, tiled) &&
                  offsetof(zs_exr_info, tile_w) == offsetof(ExrInfo, tile_w),
              "zs_exr_info mirrors ExrInfo");
static_assert(sizeof(zs_exr_channel) == sizeof(ExrChannel) && offsetof(zs_exr_channel, plane_off) == offsetof(ExrChannel, plane_off), "zs_exr_channel mirrors ExrChannel");
static_assert(sizeof(zs_exr_chunk) == sizeof(ExrChunk) && offsetof(zs_exr_chunk, status) == offsetof(ExrChunk, status) && offsetof(zs_exr_chunk, h) == offsetof(ExrChunk, h),
              "zs_exr_chunk mirrors ExrChunk");
static_assert(sizeof(ExrJob) % 8 == 0 && sizeof(ExrRun) == 16, "the jobs lie in front of the tile list, the runs behind it");

constexpr PngGrid kExrGrid{kPngSlice, kExrTilesPerWg, 64};

// One KE launch: the chunks, their runs, and the flat list of their tiles.
struct ExrSet {
    std::vector<ExrJob> jobs;
    std::vector<ExrRun> runs;
    PngOffsets tiles;
    bool sums = false;  // a chunk of the set needs the reduce launch
    // a chunk of `len` stored bytes at t; its runs follow
    void chunk(const void *t, int64_t len, bool plain) {
        jobs.push_back(ExrJob{(uint8_t *)t, (int32_t)len, (int32_t)runs.size(), 0, plain ? 1 : 0});
        tiles.add(exr_tiles(len));
        at = 0;
    }
    void run(const void *p, int64_t len) {
        runs.push_back(ExrRun{(uint8_t *)p, (int32_t)at, (int32_t)len});
        jobs.back().n_runs++, at += len;
    }
    // the runs of the part [x, x + w) x [y, y + h) of an image of width W whose channel planes begin at base + plane_off[c]
    void plane_runs(const void *base, const int64_t *plane_off, const int *sample_bytes, int n_ch, int64_t W, int64_t x, int64_t y, int64_t w, int64_t h) {
        for (int64_t r = 0; r < h; r++)
            for (int c = 0; c < n_ch; c++) run((const uint8_t *)base + plane_off[c] + ((y + r) * W + x) * sample_bytes[c], w * sample_bytes[c]);
    }
    int64_t at = 0;
};

// KE over the set on `s` (png_run_list: one wait, for the upload): the reduce launch where sums are undone, then the kernel
bool exr_run(zs_ctx *c, ExrSet &set, bool forward, hipStream_t s, bool *no_memory) {
    *no_memory = false;
    const int m = (int)set.jobs.size();
    if (m == 0) return true;
    if (set.tiles.total > kExrGrid.slice || set.runs.size() > 0x7FFFFFFFu) {
        c->err = "stream error: more than 2^25 tiles of 32 KiB or 2^31 - 1 rows of a channel in one call (split the batch)";
        return false;
    }
    const bool reduce = !forward && set.sums;
    if (reduce && !ensure(c, c->png[kBufExrSegs], 2 * (size_t)set.tiles.total)) {
        *no_memory = true;
        return false;
    }
    uint8_t *d_seg = (uint8_t *)c->png[kBufExrSegs].p;
    const size_t b_job = sizeof(ExrJob) * (size_t)m, b_off = set.tiles.bytes(true);
    return png_run_list(c, c->png[kBufExrDesc], {{set.jobs.data(), b_job}, {set.runs.data(), sizeof(ExrRun) * set.runs.size()}}, set.tiles, 0, kExrGrid, s, no_memory, nullptr,
                        [&](dim3 grid, dim3 block, uint8_t *d, int64_t row0) {
                            const ExrJob *d_job = (const ExrJob *)d;
                            const int32_t *d_off = (const int32_t *)(d + b_job);
                            const ExrRun *d_run = (const ExrRun *)(d + b_job + b_off);
                            if (forward) {
                                hipLaunchKernelGGL(zs_exr_predict_kernel, grid, block, 0, s, d_job, d_off, m, row0, d_run);
                            } else {
                                if (reduce) hipLaunchKernelGGL(zs_exr_reduce_kernel, grid, block, 0, s, d_job, d_off, m, row0, d_seg);
                                hipLaunchKernelGGL(zs_exr_undo_kernel, grid, block, 0, s, d_job, d_off, m, row0, d_run, (const uint8_t *)d_seg);
                            }
                        });
}

int exr_kernel_call(zs_ctx *c, int n, const void *const *in, void *const *out, const int64_t *len, bool forward, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!in || !out || !len) return ZS_STREAM_ERROR;
    for (int i = 0; i < n; i++)
        if (!in[i] || !out[i] || len[i] < 1 || len[i] > 0x7FFFFFFF) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    ExrSet set;
    set.sums = true;
    for (int i = 0; i < n; i++) {
        set.chunk(forward ? out[i] : in[i], len[i], false);
        set.run(forward ? in[i] : out[i], len[i]);
    }
    bool no_memory = false;
    if (!exr_run(c, set, forward, s, &no_memory)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    return png_done(hip_stream, s);
}

// what a zs_exr_put is written as; false for one the writer refuses
bool exr_layout(const zs_exr_put &p, ExrLayout *l, int64_t *plane_off, int *sample_bytes, int64_t *out_len) {
    if (!p.planes || p.width < 1 || p.height < 1 || p.width > 0x7FFFFFFF || p.height > 0x7FFFFFFF) return false;
    if ((int64_t)p.x_min + p.width - 1 > 0x7FFFFFFF || (int64_t)p.y_min + p.height - 1 > 0x7FFFFFFF) return false;
    if (p.n_channels < 1 || p.n_channels > kExrMaxChannels || !p.names || !p.types) return false;
    if (!(p.compression == 0 || p.compression == 2 || p.compression == 3)) return false;
    if (p.extra_len < 0 || p.extra_len > kExrMaxLen || (p.extra_len > 0 && !p.extra)) return false;
    if (p.width > kExrMaxLen / p.height) return false;
    int64_t end = 0, bpp = 0;
    for (int k = 0; k < p.n_channels; k++) {
        if (!p.names[k] || p.types[k] < 0 || p.types[k] > 2) return false;
        const size_t n = strnlen(p.names[k], 32);
        if (n < 1 || n > 31) return false;
        if (k && strcmp(p.names[k - 1], p.names[k]) >= 0) return false;  // (sorted byte-wise, and no name twice)
        const int64_t off = (end + 15) & ~(int64_t)15;
        sample_bytes[k] = exr_type_bytes(p.types[k]), plane_off[k] = off;
        end = off + p.width * p.height * sample_bytes[k], bpp += sample_bytes[k];
        if (end > kExrMaxLen) return false;
    }
    *out_len = end;
    l->width = p.width, l->height = p.height, l->x_min = p.x_min, l->y_min = p.y_min, l->n_channels = p.n_channels, l->compression = p.compression;
    l->names = p.names, l->types = p.types, l->extra = (const uint8_t *)p.extra, l->extra_len = p.extra_len;
    l->bpp = bpp, l->n_chunks = exr_ceil_div(p.height, exr_lines(p.compression));
    return l->n_chunks <= (1 << 24);
}
}  // namespace

extern "C" int zs_exr_file_info(const void *file, int64_t len, zs_exr_info *info, zs_exr_channel *channels, int64_t channels_cap, zs_exr_chunk *chunks, int64_t chunks_cap) {
    if (!file || !info || len < 0 || channels_cap < 0 || chunks_cap < 0 || (channels_cap > 0 && !channels) || (chunks_cap > 0 && !chunks)) return ZS_STREAM_ERROR;
    ExrInfo ei;
    const int rc = exr_walk((const uint8_t *)file, len, &ei, (ExrChannel *)channels, channels_cap, (ExrChunk *)chunks, chunks_cap);
    memcpy(info, &ei, sizeof ei);
    if (rc != kExrOk) return exr_err_status(rc);
    for (int64_t k = 0; k < ei.n_chunks && k < chunks_cap; k++) chunks[k].pad = 0;
    return (channels && channels_cap < ei.n_channels) || (chunks && chunks_cap < ei.n_chunks) ? ZS_BUF_ERROR : ZS_OK;
}

extern "C" int zs_exr_unpredict_batch_device(zs_ctx *c, int n, const void *const *in, void *const *out, const int64_t *len, void *hip_stream) {
    return exr_kernel_call(c, n, in, out, len, false, hip_stream);
}

extern "C" int zs_exr_predict_batch_device(zs_ctx *c, int n, const void *const *in, void *const *out, const int64_t *len, void *hip_stream) {
    return exr_kernel_call(c, n, in, out, len, true, hip_stream);
}

extern "C" int zs_exr_decode_files_batch(zs_ctx *c, int n, const void *const *file, const int64_t *file_len, void *const *out, const int64_t *out_cap, int64_t *out_len,
                                         int *const *chunk_status, int *status, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!file || !file_len || !out || !out_cap || !out_len) return ZS_STREAM_ERROR;
    for (int i = 0; i < n; i++)
        if (!file[i] || !out[i] || file_len[i] < 0 || out_cap[i] < 0) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
    const StageLayout lay(n, file_len, kExrMaxLen);  // (a larger file fails below, for itself)
    CallGate gate(n, status);
    if (!gate.open(c, hip_stream, out_len)) return ZS_STREAM_ERROR;
    hipStream_t s = gate.s;
    PartCodes pc(gate.st);
    uint8_t *d_files = nullptr;
    if (const int rc = stage_files(c, lay, file, file_len, s, &d_files)) return gate.fail_all(rc);
    // ---- the walk: every file's header, every chunk's place and route
    struct Ref {
        int file, chunk;
        int64_t buf;  // its place in the context's buffer
    };
    std::vector<ExrInfo> infos((size_t)n);
    std::vector<std::vector<ExrChannel>> chans((size_t)n);
    std::vector<std::vector<ExrChunk>> chunks((size_t)n);
    std::vector<Ref> inflated, plain;
    size_t buf_total = 0;
    for (int i = 0; i < n; i++) {
        if (file_len[i] > kExrMaxLen) {
            pc.fail_file(i, ZS_DATA_ERROR, "the file is above 2 GiB - 1 KiB");
            continue;
        }
        const uint8_t *f = (const uint8_t *)file[i];
        ExrInfo &ei = infos[(size_t)i];
        std::vector<ExrChunk> &C = chunks[(size_t)i];
        int rc = exr_walk(f, file_len[i], &ei, nullptr, 0, nullptr, 0);
        if (rc == kExrOk) {
            // (the room is checked between the two walks here, behind both in the TIFF call: each call keeps its order)
            out_len[i] = ei.out_len;
            if (out_cap[i] < ei.out_len) {
                pc.fail_file(i, ZS_BUF_ERROR, "buffer error");
                continue;
            }
            C.resize((size_t)ei.n_chunks), chans[(size_t)i].resize((size_t)ei.n_channels);
            rc = exr_walk(f, file_len[i], &ei, chans[(size_t)i].data(), ei.n_channels, C.data(), ei.n_chunks);
        }
        if (rc != kExrOk) {
            pc.fail_file(i, exr_err_status(rc), exr_err_message(rc));
            C.clear();
            continue;
        }
        pc.open_parts(i, C.size());
        for (size_t k = 0; k < C.size(); k++) {
            if (C[k].status != ZS_OK) {
                pc.fail_part(i, (int64_t)k, C[k].status, exr_err_message(C[k].reason));
                continue;
            }
            Ref r{i, (int)k, -1};
            if (C[k].data_len == C[k].raw_len) {
                plain.push_back(r);
            } else {
                r.buf = (int64_t)buf_total, buf_total += pad256((size_t)C[k].raw_len);
                inflated.push_back(r);
            }
        }
    }
    auto fail_chunk = [&](const Ref &r, int code, int msg) { pc.fail_part(r.file, r.chunk, code, inf_message(msg)); };
    if (!ensure(c, c->png[kBufExrChunks], buf_total + 256)) return gate.fail_all(ZS_MEM_ERROR);
    uint8_t *d_buf = (uint8_t *)c->png[kBufExrChunks].p;
    const std::string before = c->err;
    // ---- one raw inflate over all zlib chunks whose header the host accepts
    const int m = (int)inflated.size();
    std::vector<bool> decoded((size_t)m, false);
    std::vector<int> live;  // the streams of the launch
    std::vector<InfPart> parts;
    for (int j = 0; j < m; j++) {
        const Ref &r = inflated[(size_t)j];
        const ExrChunk &ch = chunks[(size_t)r.file][(size_t)r.chunk];
        int code = ZS_OK, msg = 0;
        if (!zlib_head_check((const uint8_t *)file[r.file] + ch.off, ch.data_len, &code, &msg)) {
            fail_chunk(r, code, msg);
            continue;
        }
        live.push_back(j);
        parts.push_back(InfPart{lay.at[(size_t)r.file] + (size_t)ch.off, ch.data_len, d_buf + r.buf, ch.raw_len, 2});
    }
    std::vector<InfResult> res;
    if (!inflate_parts(c, d_files, parts, s, &res)) return gate.fail_all(ZS_STREAM_ERROR);
    // a chunk must inflate to exactly its raw bytes: one that wants more ran out of the room they gave it
    std::vector<const void *> abuf;
    std::vector<int64_t> alen;
    std::vector<const uint8_t *> atrail;
    std::vector<int> aidx;
    for (size_t q = 0; q < live.size(); q++) {
        const Ref &r = inflated[(size_t)live[q]];
        const ExrChunk &ch = chunks[(size_t)r.file][(size_t)r.chunk];
        const PartVerdict v = part_verdict(res[q].status, res[q].msg, res[q].out_len, res[q].used, ch.data_len, kLenExact, ch.raw_len);
        if (v.cls == kPartFailed) fail_chunk(r, v.code, v.msg);
        else if (v.trailer_cut) fail_chunk(r, ZS_BUF_ERROR, kInfTruncated);
        else abuf.push_back(parts[q].out), alen.push_back(res[q].out_len), atrail.push_back((const uint8_t *)file[r.file] + ch.off + res[q].used), aidx.push_back(live[q]);
    }
    // ---- the Adler-32 of every stream that ended, in one launch, against the four bytes behind its last block
    std::vector<bool> same;
    if (!check_adlers(c, abuf, alen, atrail, s, &same)) return gate.fail_all(ZS_STREAM_ERROR);
    for (size_t a = 0; a < aidx.size(); a++) {
        if (same[a]) decoded[(size_t)aidx[a]] = true;
        else fail_chunk(inflated[(size_t)aidx[a]], ZS_DATA_ERROR, kInfBadCheck);
    }
    // ---- one KE launch: every inflated chunk from the buffer, and the chunks that lie raw from the uploaded files, both steps off
    ExrSet set;
    auto undo = [&](const Ref &r, const uint8_t *src, bool raw) {
        const ExrInfo &ei = infos[(size_t)r.file];
        const ExrChunk &ch = chunks[(size_t)r.file][(size_t)r.chunk];
        int64_t plane_off[kExrMaxChannels];
        int sample_bytes[kExrMaxChannels];
        for (int k = 0; k < ei.n_channels; k++) plane_off[k] = chans[(size_t)r.file][(size_t)k].plane_off, sample_bytes[k] = chans[(size_t)r.file][(size_t)k].sample_bytes;
        set.chunk(src, ch.raw_len, raw);
        set.plane_runs(out[r.file], plane_off, sample_bytes, ei.n_channels, ei.width, ch.x, ch.y, ch.w, ch.h);
        set.sums = set.sums || !raw;
    };
    for (int j = 0; j < m; j++)
        if (decoded[(size_t)j]) undo(inflated[(size_t)j], d_buf + inflated[(size_t)j].buf, false);
    for (const Ref &r : plain) undo(r, d_files + lay.at[(size_t)r.file] + (size_t)chunks[(size_t)r.file][(size_t)r.chunk].off, true);
    bool no_memory = false;
    if (!exr_run(c, set, false, s, &no_memory)) return gate.fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    if (png_done(hip_stream, s) != ZS_OK) return gate.fail_all(ZS_STREAM_ERROR);
    return gate.finish(pc.roll_up("file", "chunk", chunk_status, before, &c->err));
}

extern "C" int64_t zs_exr_bound(const zs_exr_put *put) {
    ExrLayout l;
    int64_t plane_off[kExrMaxChannels], out_len = 0;
    int sample_bytes[kExrMaxChannels];
    if (!put || !exr_layout(*put, &l, plane_off, sample_bytes, &out_len)) return -1;
    // a chunk's data are never longer than its raw bytes
    return exr_head_bytes(l) + 8 * l.n_chunks + put->width * put->height * l.bpp;
}

extern "C" int zs_exr_encode_batch_device(zs_ctx *c, int n, const zs_exr_put *puts, void *const *out, const int64_t *out_cap, int64_t *out_len, int *status, int level,
                                          int strategy, int hash_variant, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!puts || !out || !out_cap || !out_len) return ZS_STREAM_ERROR;
    struct Planes {
        int64_t off[kExrMaxChannels];
        int bytes[kExrMaxChannels];
    };
    std::vector<ExrLayout> lay((size_t)n);
    std::vector<Planes> planes((size_t)n);
    std::vector<int64_t> first((size_t)n + 1, 0);  // image i's chunks in the call's list
    size_t head_total = 0;
    for (int i = 0; i < n; i++) {
        int64_t len = 0;
        if (!out[i] || out_cap[i] < 0 || !exr_layout(puts[i], &lay[(size_t)i], planes[(size_t)i].off, planes[(size_t)i].bytes, &len)) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        first[(size_t)i + 1] = first[(size_t)i] + lay[(size_t)i].n_chunks;
        head_total += (size_t)exr_head_bytes(lay[(size_t)i]);
    }
    if (first[(size_t)n] > 0x7FFFFFFF / 3) {
        c->err = "stream error: too many chunks in one call (split the batch)";
        return ZS_STREAM_ERROR;
    }
    const int m = (int)first[(size_t)n];
    // chunk q of the call: its image, its rows, its bytes; the zlib streams are those of the images with compression 2 or 3
    struct Cut {
        int image;
        int64_t y, h, bytes;
        int z;  // its stream in the deflate call, -1: none
    };
    std::vector<Cut> cuts((size_t)m);
    std::vector<size_t> pred_at((size_t)m);
    std::vector<int64_t> zin_len, zcap;
    size_t pred_total = 0, z_total = 0;
    for (int i = 0; i < n; i++) {
        const ExrLayout &l = lay[(size_t)i];
        const int64_t L = exr_lines(l.compression);
        for (int64_t k = 0; k < l.n_chunks; k++) {
            const size_t q = (size_t)(first[(size_t)i] + k);
            Cut &t = cuts[q];
            t.image = i, t.y = k * L, t.h = std::min(L, l.height - t.y), t.bytes = t.h * l.width * l.bpp, t.z = -1;
            pred_at[q] = pred_total, pred_total += pad256((size_t)t.bytes);
            if (l.compression != 0) {
                t.z = (int)zin_len.size();
                zin_len.push_back(t.bytes), zcap.push_back(zs_deflate_bound(t.bytes));
                z_total += pad256((size_t)zcap.back());
            }
        }
    }
    const int mz = (int)zin_len.size();
    CallGate gate(n, status);
    if (!gate.open(c, hip_stream, out_len)) return ZS_STREAM_ERROR;
    hipStream_t s = gate.s;
    std::vector<int> &st = gate.st;
    // (both buffers in front of the first launch: deflate_parts finds its own in place)
    if (!ensure(c, c->png[kBufExrChunks], pred_total + 256) || !ensure(c, c->png[kBufExrZs], z_total + 256)) return gate.fail_all(ZS_MEM_ERROR);
    uint8_t *d_pred = (uint8_t *)c->png[kBufExrChunks].p;
    auto add = [&](ExrSet &set, size_t q, bool raw) {
        const Cut &t = cuts[q];
        const ExrLayout &l = lay[(size_t)t.image];
        set.chunk(d_pred + pred_at[q], t.bytes, raw);
        set.plane_runs(puts[t.image].planes, planes[(size_t)t.image].off, planes[(size_t)t.image].bytes, l.n_channels, l.width, 0, t.y, l.width, t.h);
    };
    bool no_memory = false;
    std::vector<void *> zout;
    std::vector<int64_t> zlen;
    if (mz) {
        // ---- one forward launch: every chunk that is to be deflated gathered, split and differenced
        ExrSet set;
        for (size_t q = 0; q < (size_t)m; q++)
            if (cuts[q].z >= 0) add(set, q, false);
        if (!exr_run(c, set, true, s, &no_memory)) return gate.fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
        // ---- one deflate call over all of them, into a buffer of the context
        std::vector<const void *> zin((size_t)mz);
        for (size_t q = 0; q < (size_t)m; q++)
            if (cuts[q].z >= 0) zin[(size_t)cuts[q].z] = d_pred + pred_at[q];
        if (const int zrc = deflate_parts(c, c->png[kBufExrZs], mz, zin.data(), zin_len.data(), zcap.data(), level, strategy, hash_variant, s, &zout, &zlen)) return gate.fail_all(zrc);
    }
    // ---- a second, small forward launch with both steps off: the chunks of the uncompressed files, and those that zlib did
    // not shrink, which are stored raw
    {
        ExrSet set;
        for (size_t q = 0; q < (size_t)m; q++)
            if (cuts[q].z < 0 || zlen[(size_t)cuts[q].z] >= cuts[q].bytes) cuts[q].z = -1, add(set, q, true);
        if (!exr_run(c, set, true, s, &no_memory)) return gate.fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    }
    // ---- the layout: every file's head on the host, from the lengths the deflate call returned; which files fit
    std::vector<uint8_t> heads(head_total + 2);
    std::vector<size_t> head_at((size_t)n);
    std::vector<int64_t> chunk_off((size_t)m), body_len((size_t)m);
    for (size_t q = 0; q < (size_t)m; q++) body_len[q] = cuts[q].z >= 0 ? zlen[(size_t)cuts[q].z] : cuts[q].bytes;
    int rc = ZS_OK;
    size_t at = 0, fit_spans = 0, fit_blob = 0;
    for (int i = 0; i < n; i++) {
        head_at[(size_t)i] = at;
        out_len[i] = exr_put_head(heads.data() + at, lay[(size_t)i], body_len.data() + first[(size_t)i], chunk_off.data() + first[(size_t)i]);
        at += (size_t)exr_head_bytes(lay[(size_t)i]);
    }
    if (mark_fit(st, out_len, out_cap, &rc, &c->err) == 0) return gate.finish(rc);
    for (int i = 0; i < n; i++)
        if (st[(size_t)i] == ZS_OK) fit_blob += (size_t)exr_head_bytes(lay[(size_t)i]) + 8 * (size_t)lay[(size_t)i].n_chunks, fit_spans += 1 + 2 * (size_t)lay[(size_t)i].n_chunks;
    // ---- one KC job.  Per file: its head (host bytes in the job's blob) copied into place, then per chunk its eight bytes of
    // header, from the blob too, and its data
    Crc32Job job;
    if (!crc32_begin(c, (int)fit_spans, fit_blob, &job, &no_memory)) return gate.fail_live(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    uint8_t *hb = job.blob;
    int sp = 0;
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        uint8_t *o = (uint8_t *)out[i];
        const int64_t hbytes = exr_head_bytes(lay[(size_t)i]);
        memcpy(hb, heads.data() + head_at[(size_t)i], (size_t)hbytes);
        job.spans[sp++] = Crc32Span{job.d_blob + (hb - job.blob), o, nullptr, hbytes, 0xFFFFFFFFu, 0, 0, 0};
        hb += hbytes;
        for (int64_t k = 0; k < lay[(size_t)i].n_chunks; k++) {
            const size_t q = (size_t)(first[(size_t)i] + k);
            exr_put32(hb, (uint32_t)(lay[(size_t)i].y_min + (int32_t)cuts[q].y)), exr_put32(hb + 4, (uint32_t)body_len[q]);
            job.spans[sp++] = Crc32Span{job.d_blob + (hb - job.blob), o + chunk_off[q], nullptr, 8, 0xFFFFFFFFu, 0, 0, 0};
            hb += 8;
            const uint8_t *src = cuts[q].z >= 0 ? (const uint8_t *)zout[(size_t)cuts[q].z] : d_pred + pred_at[q];
            job.spans[sp++] = Crc32Span{src, o + chunk_off[q] + 8, nullptr, body_len[q], 0xFFFFFFFFu, 0, 0, 0};
        }
    }
    if (!crc32_run(c, &job, s)) return gate.fail_live(ZS_STREAM_ERROR);
    if (c->profiling) c->stage_ms[kStCrc32] = job.ms;
    return gate.finish(rc);
}
