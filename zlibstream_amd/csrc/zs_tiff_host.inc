// zs_tiff_host.inc -- host side of the TIFF calls of include/zsgpu.h: whole files from host memory decoded on the device, and
// files written on the device from images that lie there.  Part of zs_engine.hip's translation unit, behind zs_parts_host.inc
// and zs_zip_host.inc: the call's gate, the staging, the zlib header's rules, the raw inflate of sub-streams, the Adler-32
// compare, the roll-up of the codes and the one deflate call are zs_parts.h's and zs_parts_host.inc's, the flat-list runner
// (png_run_list) and the KC job runner (Crc32Job) zs_png_host.inc's; the container's rules are zs_tiff.h's, the predictor
// kernels (KT) zs_tiff.hip's.

namespace {
static_assert(sizeof(zs_tiff_info) == sizeof(TiffInfo) && offsetof(zs_tiff_info, out_len) == offsetof(TiffInfo, out_len) &&
                  offsetof(zs_tiff_info, tiled) == offsetof(TiffInfo, tiled) && offsetof(zs_tiff_info, compression) == offsetof(TiffInfo, compression),
              "zs_tiff_info mirrors TiffInfo");
static_assert(sizeof(zs_tiff_chunk) == sizeof(TiffChunk) && offsetof(zs_tiff_chunk, status) == offsetof(TiffChunk, status) && offsetof(zs_tiff_chunk, h) == offsetof(TiffChunk, h),
              "zs_tiff_chunk mirrors TiffChunk");
static_assert(sizeof(TiffJob) % 8 == 0, "the jobs lie in front of the row list");

constexpr PngGrid kTiffGrid{kPngSlice, kTiffRowsPerWg, 64};

bool tiff_bits_ok(int bits) { return bits == 1 || bits == 2 || bits == 4 || bits == 8 || bits == 16 || bits == 32; }
bool tiff_format_ok(int bits, int spp, int predictor) {
    return tiff_bits_ok(bits) && spp >= 1 && spp <= kTiffMaxSpp && predictor >= 1 && predictor <= 3 && (predictor != 2 || bits >= 8) && (predictor != 3 || bits == 32);
}

// One KT launch: the chunks and the flat list of their rows.
struct TiffRun {
    std::vector<TiffJob> jobs;
    PngOffsets rows;
    // a chunk of chunk_w x chunk_h pixels at `chunk`, of which w x h lie in the image, at `place` there; `rows` rows are the launch's
    void add(const void *chunk, const void *place, int64_t image_pitch, int64_t chunk_w, int64_t w, int64_t h, int64_t n_rows, int bits, int spp, int predictor, bool swap) {
        TiffJob j{};
        j.chunk = (uint8_t *)chunk, j.image = (uint8_t *)place;
        j.nb = (int32_t)tiff_row_bytes(chunk_w, spp, bits), j.cb = (int32_t)tiff_row_bytes(w, spp, bits);
        j.chunk_pitch = j.nb, j.image_pitch = image_pitch;
        j.rows = (int32_t)n_rows, j.rows_in = (int32_t)h;
        j.sample_bytes = (uint8_t)(bits >= 8 ? bits / 8 : 1), j.spp = (uint8_t)(bits >= 8 ? spp : 1);  // (below 8 bits the bytes are copied)
        j.predictor = (uint8_t)predictor, j.swap = swap && bits > 8 && predictor != 3;  // (the float predictor's planes have an order of their own)
        if (n_rows > 0) jobs.push_back(j), rows.add(n_rows);
    }
};

// KT over the run on `s` (png_run_list: one wait, for the upload)
bool tiff_run(zs_ctx *c, TiffRun &run, bool forward, hipStream_t s, bool *no_memory) {
    *no_memory = false;
    const int m = (int)run.jobs.size();
    if (m == 0) return true;
    if (!png_rows_ok(c, run.rows.total)) return false;
    const size_t b_job = sizeof(TiffJob) * (size_t)m;
    return png_run_list(c, c->png[kBufTiffDesc], {{run.jobs.data(), b_job}}, run.rows, 0, kTiffGrid, s, no_memory, nullptr, [&](dim3 grid, dim3 block, uint8_t *d, int64_t row0) {
        const TiffJob *d_job = (const TiffJob *)d;
        const int32_t *d_off = (const int32_t *)(d + b_job);
        if (forward) hipLaunchKernelGGL(zs_tiff_predict_kernel, grid, block, 0, s, d_job, d_off, m, row0);
        else hipLaunchKernelGGL(zs_tiff_undo_kernel, grid, block, 0, s, d_job, d_off, m, row0);
    });
}

// the two kernel calls' arguments: chunks of width x height of which in_/out_ width x height are the image's
bool tiff_kernel_args_ok(zs_ctx *c, int n, const void *const *in, void *const *out, const int64_t *width, const int64_t *height, const int64_t *part_w,
                         const int64_t *part_h, const int *bits, const int *spp, const int *predictor) {
    if (!in || !out || !width || !height || !part_w || !part_h || !bits || !spp || !predictor) return false;
    for (int i = 0; i < n; i++) {
        const bool ok = in[i] && out[i] && png_dims_ok(width[i], height[i]) && part_w[i] >= 1 && part_h[i] >= 1 && part_w[i] <= width[i] && part_h[i] <= height[i] &&
                        tiff_format_ok(bits[i], spp[i], predictor[i]) && tiff_row_bytes(width[i], spp[i], bits[i]) <= kTiffMaxLen;
        if (!ok) {
            c->err = "stream error";
            return false;
        }
    }
    return true;
}

// what a zs_tiff_put is written as; false for one the writer refuses
bool tiff_layout(const zs_tiff_put &p, TiffLayout *l) {
    if (!p.pixels || !png_dims_ok(p.width, p.height) || !tiff_format_ok(p.bits, p.spp, p.predictor)) return false;
    if (p.sample_format < 1 || p.sample_format > 4 || (p.predictor == 3 && p.sample_format != 3)) return false;
    if (p.photometric < 0 || p.photometric > 65535 || p.photometric == 6) return false;
    if (p.extra_samples < 0 || p.extra_samples >= p.spp || p.extra_kind < 0 || p.extra_kind > 65535) return false;
    const bool tiled = p.tile_width != 0 || p.tile_height != 0;
    if (tiled && (p.tile_width < 16 || p.tile_height < 16 || p.tile_width % 16 || p.tile_height % 16 || p.tile_width > 0x7FFFFFF0 || p.tile_height > 0x7FFFFFF0)) return false;
    if (p.rows_per_strip < 0) return false;
    const int64_t row_bytes = tiff_row_bytes(p.width, p.spp, p.bits);
    if (row_bytes > kTiffMaxLen || p.height > kTiffMaxLen / row_bytes) return false;
    l->width = p.width, l->height = p.height, l->bits = p.bits, l->spp = p.spp, l->sample_format = p.sample_format, l->photometric = p.photometric;
    l->extra_samples = p.extra_samples, l->extra_kind = p.extra_kind, l->predictor = p.predictor, l->tiled = tiled;
    if (tiled) {
        l->chunk_w = p.tile_width, l->chunk_h = p.tile_height;
        l->across = tiff_ceil_div(p.width, p.tile_width);
        l->n_chunks = l->across * tiff_ceil_div(p.height, p.tile_height);
    } else {
        l->chunk_w = p.width, l->chunk_h = p.rows_per_strip ? std::min<int64_t>(p.rows_per_strip, p.height) : tiff_default_rows(row_bytes, p.height);
        l->across = 1, l->n_chunks = tiff_ceil_div(p.height, l->chunk_h);
    }
    const int64_t chunk_row = tiff_row_bytes(l->chunk_w, p.spp, p.bits);
    return chunk_row <= kTiffMaxLen && l->chunk_h <= kTiffMaxLen / chunk_row && l->n_chunks <= (1 << 24);
}
// chunk k of the layout: its place, the part inside the image, and the rows it is written with (a last strip is written short)
struct TiffCut {
    int64_t x, y, w, h, rows, bytes;
};
TiffCut tiff_cut(const TiffLayout &l, int64_t k) {
    TiffCut t;
    t.x = (k % l.across) * l.chunk_w, t.y = (k / l.across) * l.chunk_h;
    t.w = std::min(l.chunk_w, l.width - t.x), t.h = std::min(l.chunk_h, l.height - t.y);
    t.rows = l.tiled ? l.chunk_h : t.h;
    t.bytes = t.rows * tiff_row_bytes(l.chunk_w, l.spp, l.bits);
    return t;
}
}  // namespace

extern "C" int zs_tiff_file_info(const void *file, int64_t len, int64_t page, zs_tiff_info *info, zs_tiff_chunk *chunks, int64_t chunks_cap) {
    if (!file || !info || len < 0 || page < 0 || chunks_cap < 0 || (chunks_cap > 0 && !chunks)) return ZS_STREAM_ERROR;
    TiffInfo ti;
    const int rc = tiff_walk((const uint8_t *)file, len, page, &ti, (TiffChunk *)chunks, chunks_cap);
    memcpy(info, &ti, sizeof ti);
    if (rc != kTiffOk) return tiff_err_status(rc);
    return chunks && chunks_cap < ti.n_chunks ? ZS_BUF_ERROR : ZS_OK;
}

extern "C" int zs_tiff_unpredict_batch_device(zs_ctx *c, int n, const void *const *in, void *const *out, const int64_t *width, const int64_t *height,
                                              const int64_t *out_width, const int64_t *out_height, const int *bits, const int *spp, const int *predictor,
                                              const int *big_endian, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!tiff_kernel_args_ok(c, n, in, out, width, height, out_width, out_height, bits, spp, predictor)) return ZS_STREAM_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    TiffRun run;
    for (int i = 0; i < n; i++)
        run.add(in[i], out[i], tiff_row_bytes(out_width[i], spp[i], bits[i]), width[i], out_width[i], out_height[i], out_height[i], bits[i], spp[i], predictor[i],
                big_endian && big_endian[i]);
    bool no_memory = false;
    if (!tiff_run(c, run, false, s, &no_memory)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    return png_done(hip_stream, s);
}

extern "C" int zs_tiff_predict_batch_device(zs_ctx *c, int n, const void *const *in, void *const *out, const int64_t *in_width, const int64_t *in_height,
                                            const int64_t *width, const int64_t *height, const int *bits, const int *spp, const int *predictor, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!tiff_kernel_args_ok(c, n, in, out, width, height, in_width, in_height, bits, spp, predictor)) return ZS_STREAM_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    TiffRun run;
    for (int i = 0; i < n; i++)
        run.add(out[i], in[i], tiff_row_bytes(in_width[i], spp[i], bits[i]), width[i], in_width[i], in_height[i], height[i], bits[i], spp[i], predictor[i], false);
    bool no_memory = false;
    if (!tiff_run(c, run, true, s, &no_memory)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    return png_done(hip_stream, s);
}

extern "C" int zs_tiff_decode_files_batch(zs_ctx *c, int n, const void *const *file, const int64_t *file_len, const int64_t *page, void *const *out,
                                          const int64_t *out_cap, int64_t *out_len, int *const *chunk_status, int *status, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!file || !file_len || !out || !out_cap || !out_len) return ZS_STREAM_ERROR;
    for (int i = 0; i < n; i++)
        if (!file[i] || !out[i] || file_len[i] < 0 || out_cap[i] < 0 || (page && page[i] < 0)) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
    const StageLayout lay(n, file_len, kTiffMaxLen);  // (a larger file fails below, for itself)
    CallGate gate(n, status);
    if (!gate.open(c, hip_stream, out_len)) return ZS_STREAM_ERROR;
    hipStream_t s = gate.s;
    PartCodes pc(gate.st);
    uint8_t *d_files = nullptr;
    if (const int rc = stage_files(c, lay, file, file_len, s, &d_files)) return gate.fail_all(rc);
    // ---- the walk: every file's page, every chunk's place and route
    struct Ref {
        int file, chunk;
        int64_t need, full;  // the bytes its rows inside the image take, and those of the whole chunk
        int64_t buf;         // its place in the context's buffer, -1: it is decoded straight into the image
    };
    std::vector<TiffInfo> infos((size_t)n);
    std::vector<std::vector<TiffChunk>> chunks((size_t)n);
    std::vector<Ref> inflated, plain;
    size_t buf_total = 0;
    for (int i = 0; i < n; i++) {
        if (file_len[i] > kTiffMaxLen) {
            pc.fail_file(i, ZS_DATA_ERROR, "the file is above 2 GiB - 1 KiB");
            continue;
        }
        const uint8_t *f = (const uint8_t *)file[i];
        TiffInfo &ti = infos[(size_t)i];
        std::vector<TiffChunk> &C = chunks[(size_t)i];
        int rc = tiff_walk(f, file_len[i], page ? page[i] : 0, &ti, nullptr, 0);
        if (rc == kTiffOk) {
            C.resize((size_t)ti.n_chunks);
            rc = tiff_walk(f, file_len[i], page ? page[i] : 0, &ti, C.data(), ti.n_chunks);
        }
        // (the room is checked behind both walks here, between the two in the OpenEXR call: a file that the second walk refuses
        // and that has no room either gets the walk's code here and ZS_BUF_ERROR there; each call keeps its order)
        if (rc == kTiffOk) out_len[i] = ti.out_len;
        if (rc != kTiffOk) pc.fail_file(i, tiff_err_status(rc), tiff_err_message(rc));
        else if (out_cap[i] < ti.out_len) pc.fail_file(i, ZS_BUF_ERROR, "buffer error");
        if (gate.st[(size_t)i] != ZS_OK) {
            C.clear();
            continue;
        }
        pc.open_parts(i, C.size());
        const int64_t crb = tiff_row_bytes(ti.chunk_w, ti.spp, ti.bits);
        // strips of a file that needs neither sums nor swaps are the image's own bytes
        const bool own_bytes = !ti.tiled && ti.predictor == 1 && !(ti.big_endian && ti.bits > 8);
        for (size_t k = 0; k < C.size(); k++) {
            if (C[k].status != ZS_OK) {
                pc.fail_part(i, (int64_t)k, C[k].status, tiff_err_message(kTiffTruncated));
                continue;
            }
            Ref r{i, (int)k, C[k].h * crb, ti.chunk_h * crb, -1};
            if (ti.compression == 1) {
                plain.push_back(r);
            } else {
                if (!(own_bytes && r.need == r.full)) r.buf = (int64_t)buf_total, buf_total += pad256((size_t)r.full);
                inflated.push_back(r);
            }
        }
    }
    auto fail_chunk = [&](const Ref &r, int code, int msg) { pc.fail_part(r.file, r.chunk, code, inf_message(msg)); };
    auto place = [&](const Ref &r) {
        const TiffInfo &ti = infos[(size_t)r.file];
        const TiffChunk &ch = chunks[(size_t)r.file][(size_t)r.chunk];
        return (uint8_t *)out[r.file] + ch.y * ti.row_bytes + ch.x * ti.spp * ti.bits / 8;  // (a tile's x is a multiple of 16: whole bytes)
    };
    if (!ensure(c, c->png[kBufTiffChunks], buf_total + 256)) return gate.fail_all(ZS_MEM_ERROR);
    uint8_t *d_buf = (uint8_t *)c->png[kBufTiffChunks].p;
    const std::string before = c->err;
    // ---- one raw inflate over all deflated chunks whose zlib header the host accepts (Inflate.cs:211-250)
    const int m = (int)inflated.size();
    std::vector<bool> decoded((size_t)m, false);
    std::vector<int> live;  // the streams of the launch
    std::vector<InfPart> parts;
    for (int j = 0; j < m; j++) {
        const Ref &r = inflated[(size_t)j];
        const TiffChunk &ch = chunks[(size_t)r.file][(size_t)r.chunk];
        int code = ZS_OK, msg = 0;
        if (!zlib_head_check((const uint8_t *)file[r.file] + ch.off, ch.comp_len, &code, &msg)) {
            fail_chunk(r, code, msg);
            continue;
        }
        live.push_back(j);
        parts.push_back(InfPart{lay.at[(size_t)r.file] + (size_t)ch.off, ch.comp_len, r.buf < 0 ? place(r) : d_buf + r.buf, r.buf < 0 ? r.need : r.full, 2});
    }
    std::vector<InfResult> res;
    if (!inflate_parts(c, d_files, parts, s, &res)) return gate.fail_all(ZS_STREAM_ERROR);
    // a chunk longer than its rows ran out of the room they gave it; a strip must hold its rows inside the image (a last strip
    // may hold all of RowsPerStrip), a tile all of itself
    std::vector<const void *> abuf;
    std::vector<int64_t> alen;
    std::vector<const uint8_t *> atrail;
    std::vector<int> aidx;
    for (size_t q = 0; q < live.size(); q++) {
        const Ref &r = inflated[(size_t)live[q]];
        const TiffChunk &ch = chunks[(size_t)r.file][(size_t)r.chunk];
        const PartVerdict v = part_verdict(res[q].status, res[q].msg, res[q].out_len, res[q].used, ch.comp_len, kLenAtLeast, infos[(size_t)r.file].tiled ? r.full : r.need);
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
    // ---- one KT launch: every chunk that went through the buffer, and the uncompressed ones from the uploaded files
    TiffRun run;
    auto undo = [&](const Ref &r, const uint8_t *src) {
        const TiffInfo &ti = infos[(size_t)r.file];
        const TiffChunk &ch = chunks[(size_t)r.file][(size_t)r.chunk];
        run.add(src, place(r), ti.row_bytes, ti.chunk_w, ch.w, ch.h, ch.h, ti.bits, ti.spp, ti.predictor, ti.big_endian != 0);
    };
    for (int j = 0; j < m; j++)
        if (decoded[(size_t)j] && inflated[(size_t)j].buf >= 0) undo(inflated[(size_t)j], d_buf + inflated[(size_t)j].buf);
    for (const Ref &r : plain) {
        const TiffChunk &ch = chunks[(size_t)r.file][(size_t)r.chunk];
        if (ch.comp_len < (infos[(size_t)r.file].tiled ? r.full : r.need)) fail_chunk(r, ZS_DATA_ERROR, kInfBadLength);
        else undo(r, d_files + lay.at[(size_t)r.file] + (size_t)ch.off);
    }
    bool no_memory = false;
    if (!tiff_run(c, run, false, s, &no_memory)) return gate.fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    if (png_done(hip_stream, s) != ZS_OK) return gate.fail_all(ZS_STREAM_ERROR);
    return gate.finish(pc.roll_up("file", "chunk", chunk_status, before, &c->err));
}

extern "C" int64_t zs_tiff_bound(const zs_tiff_put *put) {
    TiffLayout l;
    if (!put || !tiff_layout(*put, &l)) return -1;
    const TiffCut full = tiff_cut(l, 0), last = tiff_cut(l, l.n_chunks - 1);
    const int64_t b = tiff_head_bytes(l) + (l.n_chunks - 1) * (zs_deflate_bound(full.bytes) + 1) + zs_deflate_bound(last.bytes) + 1;
    return b > 0xFFFFFFFFll ? -1 : b;  // (a file whose offsets need BigTIFF, which is not written)
}

extern "C" int zs_tiff_encode_batch_device(zs_ctx *c, int n, const zs_tiff_put *puts, void *const *out, const int64_t *out_cap, int64_t *out_len, int *status,
                                           int level, int strategy, int hash_variant, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!puts || !out || !out_cap || !out_len) return ZS_STREAM_ERROR;
    std::vector<TiffLayout> lay((size_t)n);
    std::vector<int64_t> first((size_t)n + 1, 0);  // image i's chunks in the call's list
    size_t pred_total = 0, z_total = 0, head_total = 0;  // (z_total: the room that deflate_parts lays the streams out in)
    for (int i = 0; i < n; i++) {
        if (!out[i] || out_cap[i] < 0 || zs_tiff_bound(puts + i) < 0 || !tiff_layout(puts[i], &lay[(size_t)i])) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        first[(size_t)i + 1] = first[(size_t)i] + lay[(size_t)i].n_chunks;
    }
    if (first[(size_t)n] > 0x7FFFFFFF / 3) {
        c->err = "stream error: too many strips or tiles in one call (split the batch)";
        return ZS_STREAM_ERROR;
    }
    const int m = (int)first[(size_t)n];
    std::vector<int64_t> zin_len((size_t)m), zcap((size_t)m);
    std::vector<size_t> pred_at((size_t)m);
    for (int i = 0; i < n; i++) {
        for (int64_t k = 0; k < lay[(size_t)i].n_chunks; k++) {
            const size_t q = (size_t)(first[(size_t)i] + k);
            zin_len[q] = tiff_cut(lay[(size_t)i], k).bytes, zcap[q] = zs_deflate_bound(zin_len[q]);
            pred_at[q] = pred_total, pred_total += pad256((size_t)zin_len[q]), z_total += pad256((size_t)zcap[q]);
        }
        head_total += (size_t)tiff_head_bytes(lay[(size_t)i]);
    }
    CallGate gate(n, status);
    if (!gate.open(c, hip_stream, out_len)) return ZS_STREAM_ERROR;
    hipStream_t s = gate.s;
    std::vector<int> &st = gate.st;
    // (both buffers in front of the first launch: deflate_parts finds its own in place)
    if (!ensure(c, c->png[kBufTiffChunks], pred_total + 256) || !ensure(c, c->png[kBufTiffZs], z_total + 256)) return gate.fail_all(ZS_MEM_ERROR);
    uint8_t *d_pred = (uint8_t *)c->png[kBufTiffChunks].p;
    // ---- one forward launch: every chunk of every image cut, padded and predicted
    TiffRun run;
    for (int i = 0; i < n; i++) {
        const TiffLayout &l = lay[(size_t)i];
        const int64_t row_bytes = tiff_row_bytes(l.width, l.spp, l.bits);
        for (int64_t k = 0; k < l.n_chunks; k++) {
            const TiffCut t = tiff_cut(l, k);
            run.add(d_pred + pred_at[(size_t)(first[(size_t)i] + k)], (const uint8_t *)puts[i].pixels + t.y * row_bytes + t.x * l.spp * l.bits / 8, row_bytes, l.chunk_w,
                    t.w, t.h, t.rows, l.bits, l.spp, l.predictor, false);
        }
    }
    bool no_memory = false;
    if (!tiff_run(c, run, true, s, &no_memory)) return gate.fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    // ---- one deflate call over all of them, into a buffer of the context
    std::vector<const void *> zin((size_t)m);
    std::vector<void *> zout;
    std::vector<int64_t> zlen;
    for (int q = 0; q < m; q++) zin[(size_t)q] = d_pred + pred_at[(size_t)q];
    if (const int zrc = deflate_parts(c, c->png[kBufTiffZs], m, zin.data(), zin_len.data(), zcap.data(), level, strategy, hash_variant, s, &zout, &zlen)) return gate.fail_all(zrc);
    // ---- the layout: every file's head on the host, from the lengths the deflate call returned; which files fit
    std::vector<uint8_t> heads(head_total + 2);
    std::vector<size_t> head_at((size_t)n);
    std::vector<int64_t> chunk_off((size_t)m);
    int rc = ZS_OK;
    size_t at = 0, fit_spans = 0, fit_heads = 0;
    for (int i = 0; i < n; i++) {
        head_at[(size_t)i] = at;
        out_len[i] = tiff_put_head(heads.data() + at, lay[(size_t)i], zlen.data() + first[(size_t)i], chunk_off.data() + first[(size_t)i]);
        at += (size_t)tiff_head_bytes(lay[(size_t)i]);
    }
    if (mark_fit(st, out_len, out_cap, &rc, &c->err) == 0) return gate.finish(rc);
    for (int i = 0; i < n; i++)
        if (st[(size_t)i] == ZS_OK) fit_heads += (size_t)tiff_head_bytes(lay[(size_t)i]), fit_spans += 1 + 2 * (size_t)lay[(size_t)i].n_chunks;
    // ---- one KC job.  Per file: its head (host bytes in the job's blob) copied into place, then every chunk's stream, and behind
    // a stream of odd length one zero byte, so that the next one begins at an even offset
    Crc32Job job;
    if (!crc32_begin(c, (int)fit_spans, 16 + fit_heads, &job, &no_memory)) return gate.fail_live(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    memset(job.blob, 0, 16);  // the zero byte
    uint8_t *hb = job.blob + 16;
    int sp = 0;
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        uint8_t *o = (uint8_t *)out[i];
        const int64_t hbytes = tiff_head_bytes(lay[(size_t)i]);
        memcpy(hb, heads.data() + head_at[(size_t)i], (size_t)hbytes);
        job.spans[sp++] = Crc32Span{job.d_blob + (hb - job.blob), o, nullptr, hbytes, 0xFFFFFFFFu, 0, 0, 0};
        hb += hbytes;
        for (int64_t k = 0; k < lay[(size_t)i].n_chunks; k++) {
            const size_t q = (size_t)(first[(size_t)i] + k);
            job.spans[sp++] = Crc32Span{(const uint8_t *)zout[q], o + chunk_off[q], nullptr, zlen[q], 0xFFFFFFFFu, 0, 0, 0};
            const int64_t odd = zlen[q] & 1;  // (a span without bytes where the length is even)
            job.spans[sp++] = Crc32Span{job.d_blob, odd ? o + chunk_off[q] + zlen[q] : nullptr, nullptr, odd, 0xFFFFFFFFu, 0, 0, 0};
        }
    }
    if (!crc32_run(c, &job, s)) return gate.fail_live(ZS_STREAM_ERROR);
    if (c->profiling) c->stage_ms[kStCrc32] = job.ms;
    return gate.finish(rc);
}
