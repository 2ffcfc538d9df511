// zs_png_host.inc -- the host side of the PNG and CRC-32 entry points (included by zs_engine.hip): argument checks,
// descriptor uploads and launches of the kernels of zs_png.hip and zs_crc32.hip, and the calls built from them.

// ------------------------------------------------------------------ what the calls below share
namespace {
bool png_format_ok(zs_ctx *c, int format) {
    if (format == ZS_PNG_FMT_RGBA8 || format == ZS_PNG_FMT_RGBA16) return true;
    c->err = "stream error: format is neither ZS_PNG_RGBA8 nor ZS_PNG_RGBA16";
    return false;
}
bool png_dims_ok(int64_t w, int64_t h) { return w >= 1 && h >= 1 && w <= 0x7FFFFFFF && h <= 0x7FFFFFFF; }
bool png_rows_ok(zs_ctx *c, int64_t rows) {  // (a call's flat list is indexed with 32 bits)
    if (rows <= 0x7FFFFFFF) return true;
    c->err = "stream error: more than 2^31 - 1 rows in one call (split the batch)";
    return false;
}

// how a call ends: its launches stay in flight on the caller's stream, the context's own is waited for
int png_done(void *hip_stream, hipStream_t s) { return hip_stream ? ZS_OK : (hipStreamSynchronize(s) == hipSuccess ? ZS_OK : ZS_STREAM_ERROR); }

// profiling: the call's one stage (a call of several stages sets the others behind this)
void png_set_stage(zs_ctx *c, int stage, double ms) {
    if (!c->profiling) return;
    for (double &v : c->stage_ms) v = 0;
    c->stage_ms[stage] = ms;
}

// The flat list of a launch's items -- rows, pass rows or waves, image after image: off[i] = items of the images before i,
// and on the device one entry more, the total.
struct PngOffsets {
    std::vector<int32_t> off;
    int64_t total = 0;
    void add(int64_t items) {
        off.push_back((int32_t)total);
        total += items;
    }
    // on the device, `padded` to a multiple of 16 where something lies behind the list
    size_t bytes(bool padded) const {
        const size_t b = sizeof(int32_t) * (off.size() + 1);
        return padded ? (b + 15) & ~(size_t)15 : b;
    }
};

// A flat-list kernel's launches: `slice` items a launch (a grid holds fewer than 2^32 threads: 2^31 of them a launch, half of
// what it may hold), `per_wg` items a workgroup, `threads` threads an item.
struct PngGrid {
    int64_t slice;
    int per_wg, threads;
};
constexpr int64_t kPngSlice = 1 << 25;  // the slice of the kernels with a wave (64 threads) an item; the filter's: kPngFilterGrid

// launch(grid, block, first): one launch over the items from `first` on.  A list of more than a slice is several launches.
template <class Launch>
bool png_launch_list(zs_ctx *c, int64_t total, const PngGrid &g, Launch &&launch) {
    for (int64_t first = 0; first < total; first += g.slice) {
        const int64_t items = std::min<int64_t>(g.slice, total - first);
        launch(dim3((unsigned)((items + g.per_wg - 1) / g.per_wg)), dim3((unsigned)(g.threads * g.per_wg)), first);
        ZS_HIP(c, hipGetLastError());
    }
    return true;
}

struct PngPart {
    const void *p;
    size_t bytes;
};

// One flat-list kernel over one job.  Lays out in the staging buffer, and through one copy in `desc`: parts[0] (the
// descriptors), the list's offsets and its total, the other parts (tables, frames), `zeroed` bytes of zeros (counters).  Every
// part but the offsets is a multiple of 8 bytes, and the offsets are padded where a part follows them.  Then
// launch(grid, block, d_base, first) for every slice of the list, d_base being where parts[0] lies on the device.
// Waits for `s` once: for the upload (the staging buffer is the caller's again) and leaves the launches in flight; or, with
// profiling on and `ms` given, for the launches, whose time goes to *ms.
template <class Launch>
bool png_run_list(zs_ctx *c, DevBuf &desc, std::initializer_list<PngPart> parts, const PngOffsets &list, size_t zeroed, const PngGrid &g, hipStream_t s,
                  bool *no_memory, double *ms, Launch &&launch) {
    *no_memory = false;
    const size_t m = list.off.size(), b_off = list.bytes(parts.size() > 1 || zeroed);
    size_t b_all = b_off + zeroed;
    for (const PngPart &p : parts) b_all += p.bytes;
    if (!ensure(c, desc, b_all) || !ensure_pinned(c, b_all)) {
        *no_memory = true;
        return false;
    }
    uint8_t *hp = (uint8_t *)c->pinned;
    size_t at = 0;
    auto put = [&](const void *p, size_t bytes) {
        if (bytes) memcpy(hp + at, p, bytes);
        at += bytes;
    };
    const int32_t total = (int32_t)list.total;
    const PngPart *part = parts.begin();
    put(part->p, part->bytes);
    put(list.off.data(), sizeof(int32_t) * m), put(&total, sizeof total);
    at = part->bytes + b_off;
    for (++part; part != parts.end(); ++part) put(part->p, part->bytes);
    memset(hp + at, 0, zeroed);
    ZS_HIP(c, hipMemcpyAsync(desc.p, c->pinned, b_all, hipMemcpyHostToDevice, s));
    const bool timed = ms && c->profiling;
    if (!timed) ZS_HIP(c, hipStreamSynchronize(s));
    else (void)hipEventRecord(c->ev_png[0], s);
    uint8_t *d_base = (uint8_t *)desc.p;
    if (!png_launch_list(c, list.total, g, [&](dim3 grid, dim3 block, int64_t first) { launch(grid, block, d_base, first); })) return false;
    if (timed) {
        (void)hipEventRecord(c->ev_png[1], s);
        ZS_HIP(c, hipStreamSynchronize(s));
        float t = 0;
        (void)hipEventElapsedTime(&t, c->ev_png[0], c->ev_png[1]);
        *ms = t;
    }
    return true;
}
}  // namespace

// ------------------------------------------------------------------ PNG scanline filtering (the caller path of the sparse case)
extern "C" int zs_png_filter_device(zs_ctx *c, const void *pixels, int64_t row_bytes, int64_t height, int bpp, int filter, void *out,
                                    void *hip_stream) {
    if (!c || !pixels || !out || row_bytes <= 0 || height <= 0 || bpp < 1 || bpp > 8 || filter < 0 || filter > 5 || height > 0x7FFFFFFF)
        return ZS_STREAM_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    hipLaunchKernelGGL(zs_png_filter_kernel, dim3((unsigned)height), dim3(256), 0, s, (const uint8_t *)pixels, row_bytes, height, bpp, filter,
                       (uint8_t *)out);
    if (hipGetLastError() != hipSuccess) return ZS_STREAM_ERROR;
    return png_done(hip_stream, s);
}

// ... for a batch: one launch over the flat list of all images' rows (zs_kernels.hip zs_png_filter_batch_kernel)
namespace {
bool png_filter_args(zs_ctx *c, int n, const void *const *pixels, const int64_t *row_bytes, const int64_t *height, const int *bpp, const int *filter,
                     void *const *out, int64_t *total_rows) {
    *total_rows = 0;
    for (int i = 0; i < n; i++) {
        if (!pixels[i] || (out && !out[i]) || row_bytes[i] <= 0 || height[i] <= 0 || height[i] > 0x7FFFFFFF || bpp[i] < 1 || bpp[i] > 8 || filter[i] < 0 ||
            filter[i] > 5) {
            c->err = "stream error";
            return false;
        }
        *total_rows += height[i];
    }
    return png_rows_ok(c, *total_rows);  // (the grid is the row list)
}

constexpr PngGrid kPngFilterGrid{1 << 23, 1, 256};  // a workgroup of 256 threads a row

// the launch is left in flight on `s`; the descriptors have left the pinned staging buffer when this returns (never timed:
// the wait is the upload's, with profiling on too)
bool run_png_filter_batch(zs_ctx *c, int n, const void *const *pixels, const int64_t *row_bytes, const int64_t *height, const int *bpp, const int *filter,
                          void *const *out, hipStream_t s) {
    std::vector<PngFiltImg> img((size_t)n);
    PngOffsets list;
    list.off.reserve((size_t)n);
    for (int i = 0; i < n; i++) {
        img[(size_t)i] = PngFiltImg{(const uint8_t *)pixels[i], (uint8_t *)out[i], row_bytes[i], bpp[i], filter[i]};
        list.add(height[i]);
    }
    const size_t b_img = sizeof(PngFiltImg) * (size_t)n;
    const int stage = getenv("ZS_PNG_NO_STAGE") ? 0 : 1;
    bool no_memory = false;
    return png_run_list(c, c->png[kBufPngFimg], {{img.data(), b_img}}, list, 0, kPngFilterGrid, s, &no_memory, nullptr,
                        [&](dim3 grid, dim3 block, uint8_t *d, int64_t row0) {
                            hipLaunchKernelGGL(zs_png_filter_batch_kernel, grid, block, 0, s, (const PngFiltImg *)d, (const int32_t *)(d + b_img), n, stage, row0);
                        });
}
}  // namespace

extern "C" int zs_png_filter_batch_device(zs_ctx *c, int n, const void *const *pixels, const int64_t *row_bytes, const int64_t *height, const int *bpp,
                                          const int *filter, void *const *out, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!pixels || !row_bytes || !height || !bpp || !filter || !out) return ZS_STREAM_ERROR;
    int64_t total_rows = 0;
    if (!png_filter_args(c, n, pixels, row_bytes, height, bpp, filter, out, &total_rows)) return ZS_STREAM_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (!run_png_filter_batch(c, n, pixels, row_bytes, height, bpp, filter, out, s)) return ZS_STREAM_ERROR;
    return png_done(hip_stream, s);
}

// Pixels -> IDAT payloads: the batch filter into the context's scratch buffer, then every image's rows as the Writes of its
// own stream (rows_per_write rows a Write; 0: one Write).  Nothing leaves the device in between.
extern "C" int zs_png_idat_batch_device(zs_ctx *c, int n, const void *const *pixels, const int64_t *row_bytes, const int64_t *height, const int *bpp,
                                        const int *filter, int64_t rows_per_write, void *const *out, const int64_t *out_cap, int64_t *out_len,
                                        int *status, int level, int strategy, int hash_variant, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!pixels || !row_bytes || !height || !bpp || !filter || !out || !out_cap || !out_len || rows_per_write < 0) return ZS_STREAM_ERROR;
    for (int i = 0; i < n; i++) {
        out_len[i] = 0;
        if (status) status[i] = ZS_STREAM_ERROR;
    }
    int64_t total_rows = 0;
    if (!png_filter_args(c, n, pixels, row_bytes, height, bpp, filter, nullptr, &total_rows)) return ZS_STREAM_ERROR;
    std::vector<int64_t> len((size_t)n);
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        if (row_bytes[i] > 0x7FFFFFFF || height[i] * (row_bytes[i] + 1) > 0x7FFFFFFF - 1024) {  // (a stream's input is indexed with 32 bits)
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        len[(size_t)i] = height[i] * (row_bytes[i] + 1);
        total += ((size_t)len[(size_t)i] + 255) & ~(size_t)255;
    }
    if (!check_args(c, n, len.data(), level, strategy)) return ZS_STREAM_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (!ensure(c, c->png[kBufPngScratch], total + 256)) return ZS_MEM_ERROR;
    std::vector<void *> rows((size_t)n);
    std::vector<const void *> rows_in((size_t)n);
    std::vector<std::vector<int64_t>> ends((size_t)n);
    std::vector<const int64_t *> ends_p((size_t)n, nullptr);
    std::vector<int64_t> n_ends((size_t)n, 0);
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        rows[(size_t)i] = (uint8_t *)c->png[kBufPngScratch].p + at;
        rows_in[(size_t)i] = rows[(size_t)i];
        at += ((size_t)len[(size_t)i] + 255) & ~(size_t)255;
        if (rows_per_write > 0 && rows_per_write < height[i]) {
            for (int64_t r = rows_per_write; r < height[i]; r += rows_per_write) ends[(size_t)i].push_back(r * (row_bytes[i] + 1));
            ends[(size_t)i].push_back(len[(size_t)i]);
            ends_p[(size_t)i] = ends[(size_t)i].data(), n_ends[(size_t)i] = (int64_t)ends[(size_t)i].size();
        }
    }
    if (!run_png_filter_batch(c, n, pixels, row_bytes, height, bpp, filter, rows.data(), s)) return ZS_STREAM_ERROR;
    return zs_deflate_writes_batch_device(c, n, rows_in.data(), len.data(), ends_p.data(), n_ends.data(), out, out_cap, out_len, status, level, strategy,
                                          hash_variant, hip_stream);
}

// ------------------------------------------------------------------ PNG scanline reconstruction (KU, zs_png.hip): inflate -> pixels in HBM
namespace {
constexpr int kPngGrid = 1024;  // workgroups that loop over the segments: four per CU where the tiles allow it

// Enqueue: the descriptors' upload, the scan, KU and the counters' way back to the staging buffer, all left in flight on `s`.
// pinned_extra: bytes of the staging buffer the caller wants for itself behind this call's share, at *pinned_extra_at (the
// buffer is sized once, here: growing it would move it under the copies in flight).
bool png_unfilter_enqueue(zs_ctx *c, int n, const void *const *in, const int64_t *row_bytes, const int64_t *height, const int *bpp, void *const *out,
                          int64_t total_rows, int max_bpp, hipStream_t s, bool *no_memory, size_t pinned_extra = 0, size_t *pinned_extra_at = nullptr) {
    const size_t b_img = sizeof(PngImg) * (size_t)n, b_ctr = sizeof(int32_t) * ((size_t)n + 1);
    const size_t b_own = (std::max(b_img, b_ctr) + 255) & ~(size_t)255;
    if (!ensure(c, c->png[kBufPngImg], b_img) || !ensure(c, c->png[kBufPngSeg], sizeof(PngSeg) * (size_t)total_rows) || !ensure(c, c->png[kBufPngCtr], b_ctr) ||
        !ensure_pinned(c, pinned_extra ? b_own + pinned_extra : std::max(b_img, b_ctr))) {
        *no_memory = true;
        return false;
    }
    if (pinned_extra_at) *pinned_extra_at = b_own;
    PngImg *hi = (PngImg *)c->pinned;
    for (int i = 0; i < n; i++) hi[i] = PngImg{(const uint8_t *)in[i], (uint8_t *)out[i], row_bytes[i], (int32_t)height[i], bpp[i]};
    ZS_HIP(c, hipMemcpyAsync(c->png[kBufPngImg].p, c->pinned, b_img, hipMemcpyHostToDevice, s));
    ZS_HIP(c, hipMemsetAsync(c->png[kBufPngCtr].p, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(zs_png_scan_kernel, dim3((unsigned)n), dim3(256), 0, s, (const PngImg *)c->png[kBufPngImg].p, (PngSeg *)c->png[kBufPngSeg].p, (int32_t *)c->png[kBufPngCtr].p);
    ZS_HIP(c, hipGetLastError());
    const int waves = png_waves(max_bpp);
    const int tiles = waves * kPngRows * png_tile_stride(max_bpp);
    hipLaunchKernelGGL(zs_png_unfilter_kernel, dim3((unsigned)std::min<int64_t>(total_rows, kPngGrid)), dim3(64 * (unsigned)waves),
                       (size_t)png_lds_bytes(max_bpp, waves), s, (const PngImg *)c->png[kBufPngImg].p, (const PngSeg *)c->png[kBufPngSeg].p, (const int32_t *)c->png[kBufPngCtr].p, tiles);
    ZS_HIP(c, hipGetLastError());
    ZS_HIP(c, hipMemcpyAsync(c->pinned, c->png[kBufPngCtr].p, b_ctr, hipMemcpyDeviceToHost, s));  // (the descriptors' upload is through by then: same stream)
    return true;
}

// Collect, once `s` has been waited for: the statuses, the first bad row of every image (bad_row, may be null;
// kPngNoBadRow: none) and the first failing image's message.
bool png_unfilter_collect(zs_ctx *c, int n, int *st, int32_t *bad_row = nullptr) {
    const int32_t *hc = (const int32_t *)c->pinned;
    c->png_segments = hc[0];
    bool ok = true;
    for (int i = n - 1; i >= 0; i--) {
        st[i] = hc[1 + i] == kPngNoBadRow ? ZS_OK : ZS_DATA_ERROR;
        if (bad_row) bad_row[i] = hc[1 + i];
        if (st[i] != ZS_OK) {
            char msg[128];
            snprintf(msg, sizeof msg, "data error: image %d: row %d has a filter type above 4", i, (int)hc[1 + i]);
            c->err = msg;  // (the loop runs downwards: the first failing image's message stays)
            ok = false;
        }
    }
    return ok;
}

bool run_png_unfilter(zs_ctx *c, int n, const void *const *in, const int64_t *row_bytes, const int64_t *height, const int *bpp, void *const *out,
                      int64_t total_rows, int max_bpp, int *st, hipStream_t s, bool *no_memory) {
    if (!png_unfilter_enqueue(c, n, in, row_bytes, height, bpp, out, total_rows, max_bpp, s, no_memory)) return false;
    ZS_HIP(c, hipStreamSynchronize(s));
    return png_unfilter_collect(c, n, st);
}
}  // namespace

extern "C" int zs_png_unfilter_batch_device(zs_ctx *c, int n, const void *const *in, const int64_t *row_bytes, const int64_t *height, const int *bpp,
                                            void *const *out, int *status, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!in || !row_bytes || !height || !bpp || !out) return ZS_STREAM_ERROR;
    if (status)
        for (int i = 0; i < n; i++) status[i] = ZS_STREAM_ERROR;
    int64_t total_rows = 0;
    int max_bpp = 1;
    for (int i = 0; i < n; i++) {
        if (!in[i] || !out[i] || row_bytes[i] <= 0 || height[i] <= 0 || height[i] > 0x7FFFFFFF || bpp[i] < 1 || bpp[i] > 8) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        total_rows += height[i];
        max_bpp = std::max(max_bpp, bpp[i]);
    }
    if (!png_rows_ok(c, total_rows)) return ZS_STREAM_ERROR;  // (the segment list is indexed with 32 bits)
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    std::vector<int> st((size_t)n, ZS_STREAM_ERROR);
    bool no_memory = false;
    const bool ok = run_png_unfilter(c, n, in, row_bytes, height, bpp, out, total_rows, max_bpp, st.data(), s, &no_memory);
    if (no_memory) std::fill(st.begin(), st.end(), (int)ZS_MEM_ERROR);  // (the workspace or the staging buffer did not fit: not the caller's arguments)
    if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
    if (ok) return ZS_OK;
    for (int v : st)
        if (v != ZS_OK) return v;
    return ZS_STREAM_ERROR;
}

extern "C" int zs_png_unfilter_device(zs_ctx *c, const void *in, int64_t row_bytes, int64_t height, int bpp, void *out, void *hip_stream) {
    return zs_png_unfilter_batch_device(c, 1, &in, &row_bytes, &height, &bpp, &out, nullptr, hip_stream);
}

// ------------------------------------------------------------------ Adam7 (KA, zs_png.hip) and the decode call: IDAT payloads -> pixels in HBM
extern "C" int64_t zs_png_idat_layout(int64_t width, int64_t height, int bits_per_pixel, int interlace, int64_t *row_bytes7, int64_t *rows7) {
    if (!png_dims_ok(width, height) || !png_bits_ok(bits_per_pixel) || (interlace != 0 && interlace != 1)) return -1;
    int64_t total = 0;
    for (int p = 0; p < kAdam7Passes; p++) {
        int64_t pw = 0, ph = 0;
        if (interlace) pw = adam7_pass_width(width, p), ph = adam7_pass_height(height, p);
        else if (p == 0) pw = width, ph = height;
        const bool present = pw > 0 && ph > 0;
        const int64_t rb = present ? png_bits_row_bytes(pw, bits_per_pixel) : 0, rows = present ? ph : 0;
        if (row_bytes7) row_bytes7[p] = rb;
        if (rows7) rows7[p] = rows;
        total += rows * (rb + 1);  // (below 2^31 * (2^34 + 1) a pass: seven of them fit 64 bits)
    }
    return total;
}

namespace {
constexpr PngGrid kAdam7Grid{kPngSlice, kAdam7RowsPerWg, 64};

// `staged`: m Adam7Img and then the m + 1 row offsets, in the context's staging buffer.  Left in flight on `s`.
// wait_upload: the caller does not wait for `s` itself before the staging buffer is used again.
bool png_adam7_enqueue(zs_ctx *c, int m, const void *staged, int64_t total_rows, hipStream_t s, bool wait_upload) {
    const size_t b_img = sizeof(Adam7Img) * (size_t)m, b_off = sizeof(int32_t) * ((size_t)m + 1);
    ZS_HIP(c, hipMemcpyAsync(c->png[kBufPngA7img].p, staged, b_img + b_off, hipMemcpyHostToDevice, s));
    if (wait_upload) ZS_HIP(c, hipStreamSynchronize(s));
    static const int group = getenv("ZS_PNG_A7_GROUP") ? atoi(getenv("ZS_PNG_A7_GROUP")) : 16;  // (measurements: DESIGN.md section 4, KA)
    const Adam7Img *d_img = (const Adam7Img *)c->png[kBufPngA7img].p;
    const int32_t *d_off = (const int32_t *)((const uint8_t *)c->png[kBufPngA7img].p + b_img);
    return png_launch_list(c, total_rows, kAdam7Grid, [&](dim3 grid, dim3 block, int64_t row0) {
        if (group == 4) hipLaunchKernelGGL(zs_png_adam7_kernel<4>, grid, block, 0, s, d_img, d_off, m, row0);
        else if (group == 8) hipLaunchKernelGGL(zs_png_adam7_kernel<8>, grid, block, 0, s, d_img, d_off, m, row0);
        else hipLaunchKernelGGL(zs_png_adam7_kernel<16>, grid, block, 0, s, d_img, d_off, m, row0);
    });
}
size_t png_adam7_staged_bytes(int m) { return sizeof(Adam7Img) * (size_t)m + sizeof(int32_t) * ((size_t)m + 1); }
}  // namespace

extern "C" int zs_png_adam7_merge_batch_device(zs_ctx *c, int n, const void *const *passes, const int64_t *width, const int64_t *height,
                                               const int *bits_per_pixel, void *const *out, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!passes || !width || !height || !bits_per_pixel || !out) return ZS_STREAM_ERROR;
    int64_t total_rows = 0;
    for (int i = 0; i < n; i++) {
        if (!passes[i] || !out[i] || !png_dims_ok(width[i], height[i]) || !png_bits_ok(bits_per_pixel[i])) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        total_rows += height[i];
    }
    if (!png_rows_ok(c, total_rows)) return ZS_STREAM_ERROR;  // (the grid is the row list)
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const size_t bytes = png_adam7_staged_bytes(n);
    if (!ensure(c, c->png[kBufPngA7img], bytes) || !ensure_pinned(c, bytes)) return ZS_MEM_ERROR;
    Adam7Img *hi = (Adam7Img *)c->pinned;
    int32_t *ho = (int32_t *)((uint8_t *)c->pinned + sizeof(Adam7Img) * (size_t)n);
    int64_t at = 0;
    for (int i = 0; i < n; i++) {
        hi[i] = Adam7Img{(const uint8_t *)passes[i], (uint8_t *)out[i], {}, (int32_t)width[i], (int32_t)height[i], bits_per_pixel[i], 0};
        adam7_layout(hi[i]);
        ho[i] = (int32_t)at;
        at += height[i];
    }
    ho[n] = (int32_t)at;
    if (!png_adam7_enqueue(c, n, c->pinned, total_rows, s, true)) return ZS_STREAM_ERROR;
    return png_done(hip_stream, s);
}

// Inflate into a buffer of the context, KU over every image or present pass whose stream gave exactly what the IHDR needs,
// KA behind it on the same stream for the interlaced ones.  Two waits: inflate's results decide what KU may touch.
extern "C" int zs_png_decode_batch_device(zs_ctx *c, int n, const void *const *idat, const int64_t *idat_len, const int64_t *width, const int64_t *height,
                                          const int *bits_per_pixel, const int *interlace, void *const *out, int *status, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!idat || !idat_len || !width || !height || !bits_per_pixel || !interlace || !out) return ZS_STREAM_ERROR;
    constexpr int64_t kLim = 0x7FFFFFFF - 1024;  // what one inflate stream may take and give
    std::vector<int64_t> need((size_t)n), inf_at((size_t)n), pass_at((size_t)n, 0);
    int64_t total_rows = 0, n_items = 0, n_a7 = 0, a7_rows = 0;
    size_t inf_total = 0, pass_total = 0;
    for (int i = 0; i < n; i++) {
        int64_t rb7[kAdam7Passes], rows7[kAdam7Passes];
        need[(size_t)i] = !idat[i] || !out[i] || idat_len[i] < 0 || idat_len[i] > kLim
                              ? -1
                              : zs_png_idat_layout(width[i], height[i], bits_per_pixel[i], interlace[i], rb7, rows7);
        if (need[(size_t)i] < 0 || need[(size_t)i] > kLim) {
            c->err = need[(size_t)i] > kLim ? "stream error: an image's IDAT payload is above 2 GiB - 1 KiB" : "stream error";
            return ZS_STREAM_ERROR;
        }
        inf_at[(size_t)i] = (int64_t)inf_total;
        inf_total += ((size_t)need[(size_t)i] + 255) & ~(size_t)255;
        int64_t px = 0;
        for (int p = 0; p < kAdam7Passes; p++) total_rows += rows7[p], n_items += rows7[p] > 0, px += rb7[p] * rows7[p];
        if (interlace[i]) {
            pass_at[(size_t)i] = (int64_t)pass_total;
            pass_total += ((size_t)px + 255) & ~(size_t)255;
            n_a7++, a7_rows += height[i];
        }
    }
    if (total_rows > 0x7FFFFFFF) {  // (KU's segment list and KA's row list are indexed with 32 bits)
        c->err = "stream error: more than 2^31 - 1 rows in one call, pass rows counted (split the batch)";
        return ZS_STREAM_ERROR;
    }
    std::vector<int> st((size_t)n, ZS_STREAM_ERROR);
    auto finish = [&](int rc) {
        if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
        return rc;
    };
    if (hipSetDevice(c->device) != hipSuccess) return finish(ZS_STREAM_ERROR);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (!ensure(c, c->png[kBufPngInflated], inf_total + 256) || !ensure(c, c->png[kBufPngPasses], pass_total + 256) ||
        (n_a7 && !ensure(c, c->png[kBufPngA7img], png_adam7_staged_bytes((int)n_a7)))) {
        std::fill(st.begin(), st.end(), (int)ZS_MEM_ERROR);
        return finish(ZS_MEM_ERROR);
    }
    // ---- inflate: every stream against exactly the bytes its image needs
    std::vector<void *> inf_out((size_t)n);
    std::vector<int64_t> got((size_t)n, 0);
    std::vector<int> ist((size_t)n, ZS_STREAM_ERROR);
    for (int i = 0; i < n; i++) inf_out[(size_t)i] = (uint8_t *)c->png[kBufPngInflated].p + inf_at[(size_t)i];
    const int inf_rc = zs_inflate_batch_device(c, n, idat, idat_len, inf_out.data(), need.data(), got.data(), ist.data(), (void *)s);
    const std::string inf_msg = inf_rc == ZS_OK ? std::string() : c->err;
    for (int v : ist)
        if (v == ZS_STREAM_ERROR || v == ZS_MEM_ERROR) return finish(v);  // (the device or the workspace failed, not a stream)
    // what went wrong with image i, if anything did so far
    std::vector<std::string> why((size_t)n);
    char msg[192];
    for (int i = 0; i < n; i++) {
        const int64_t nd = need[(size_t)i];
        if (ist[(size_t)i] == ZS_STREAM_END && got[(size_t)i] == nd) continue;
        if (ist[(size_t)i] == ZS_STREAM_END)
            snprintf(msg, sizeof msg, "data error: image %d: IDAT holds %lld bytes, the image needs %lld", i, (long long)got[(size_t)i], (long long)nd);
        else if (ist[(size_t)i] == ZS_BUF_ERROR)
            snprintf(msg, sizeof msg, "data error: image %d: IDAT holds more than the %lld bytes the image needs, or its stream is cut short (%lld bytes came out)", i,
                     (long long)nd, (long long)got[(size_t)i]);
        else snprintf(msg, sizeof msg, "data error: image %d: %s", i, inf_msg.c_str());
        why[(size_t)i] = msg;
    }
    // ---- KU over the good images and their present passes, KA behind it
    struct Item {
        int img, pass;  // pass -1: a non-interlaced image
    };
    std::vector<Item> items;
    std::vector<const void *> u_in;
    std::vector<void *> u_out;
    std::vector<int64_t> u_rb, u_h;
    std::vector<int> u_bpp;
    std::vector<Adam7Img> a7;
    std::vector<int32_t> a7_off;
    items.reserve((size_t)n_items);
    int64_t u_rows = 0, a_rows = 0;
    int max_bpp = 1;
    for (int i = 0; i < n; i++) {
        if (!why[(size_t)i].empty()) continue;
        const int bpp = png_bits_bpp(bits_per_pixel[i]);
        max_bpp = std::max(max_bpp, bpp);
        const uint8_t *src = (const uint8_t *)inf_out[(size_t)i];
        if (!interlace[i]) {
            items.push_back(Item{i, -1});
            u_in.push_back(src), u_out.push_back(out[i]), u_rb.push_back(png_bits_row_bytes(width[i], bits_per_pixel[i])), u_h.push_back(height[i]), u_bpp.push_back(bpp);
            u_rows += height[i];
            continue;
        }
        Adam7Img im{(const uint8_t *)c->png[kBufPngPasses].p + pass_at[(size_t)i], (uint8_t *)out[i], {}, (int32_t)width[i], (int32_t)height[i], bits_per_pixel[i], 0};
        adam7_layout(im);
        for (int p = 0; p < kAdam7Passes; p++) {
            const int64_t pw = adam7_pass_width(width[i], p), ph = adam7_pass_height(height[i], p);
            if (pw == 0 || ph == 0) continue;
            const int64_t rb = png_bits_row_bytes(pw, bits_per_pixel[i]);
            items.push_back(Item{i, p});
            u_in.push_back(src), u_out.push_back(const_cast<uint8_t *>(im.passes) + im.off[p]), u_rb.push_back(rb), u_h.push_back(ph), u_bpp.push_back(bpp);
            src += ph * (rb + 1);
            u_rows += ph;
        }
        a7_off.push_back((int32_t)a_rows);
        a7.push_back(im);
        a_rows += height[i];
    }
    const int m = (int)items.size();
    std::vector<int> ust((size_t)m, ZS_OK);
    std::vector<int32_t> bad((size_t)m, kPngNoBadRow);
    if (m > 0) {
        bool no_memory = false;
        size_t extra_at = 0;
        const size_t a7_bytes = png_adam7_staged_bytes((int)a7.size());
        if (!png_unfilter_enqueue(c, m, u_in.data(), u_rb.data(), u_h.data(), u_bpp.data(), u_out.data(), u_rows, max_bpp, s, &no_memory,
                                  a7.empty() ? 0 : a7_bytes, &extra_at)) {
            if (no_memory) std::fill(st.begin(), st.end(), (int)ZS_MEM_ERROR);
            return finish(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
        }
        if (!a7.empty()) {
            a7_off.push_back((int32_t)a_rows);
            uint8_t *staged = (uint8_t *)c->pinned + extra_at;  // (behind KU's share of the staging buffer, whose results are on their way into it)
            memcpy(staged, a7.data(), sizeof(Adam7Img) * a7.size());
            memcpy(staged + sizeof(Adam7Img) * a7.size(), a7_off.data(), sizeof(int32_t) * a7_off.size());
            if (!png_adam7_enqueue(c, (int)a7.size(), staged, a_rows, s, false)) return finish(ZS_STREAM_ERROR);
        }
        if (hipStreamSynchronize(s) != hipSuccess) {
            c->err = "hipStreamSynchronize failed";
            return finish(ZS_STREAM_ERROR);
        }
        png_unfilter_collect(c, m, ust.data(), bad.data());
    }
    for (int k = m - 1; k >= 0; k--) {  // (downwards: an image's first bad pass stays)
        if (ust[(size_t)k] == ZS_OK) continue;
        const Item &it = items[(size_t)k];
        if (it.pass < 0) snprintf(msg, sizeof msg, "data error: image %d: row %d has a filter type above 4", it.img, (int)bad[(size_t)k]);
        else snprintf(msg, sizeof msg, "data error: image %d: pass %d: row %d has a filter type above 4", it.img, it.pass + 1, (int)bad[(size_t)k]);
        why[(size_t)it.img] = msg;
    }
    int rc = ZS_OK;
    for (int i = n - 1; i >= 0; i--) {
        st[(size_t)i] = why[(size_t)i].empty() ? ZS_OK : ZS_DATA_ERROR;
        if (st[(size_t)i] != ZS_OK) c->err = why[(size_t)i], rc = ZS_DATA_ERROR;  // (downwards: the first failing image's message stays)
    }
    return finish(rc);
}

// ------------------------------------------------------------------ expansion to RGBA (KX, zs_png.hip): raw scanlines -> pixels a caller can show
namespace {
constexpr PngGrid kExpandGrid{kPngSlice, kExpandRowsPerWg, 64};

// The arguments zs_png_expand_batch_device and zs_png_pack_batch_device share: `pix` is the RGBA side (aligned to a pixel),
// `raw` the scanline side.
bool png_rgba_args_ok(zs_ctx *c, int n, const void *const *pix, const void *const *raw, const int64_t *width, const int64_t *height, const int *bit_depth,
                      const int *color_type, const void *const *plte, const int *plte_entries, const void *const *trns, const int *trns_len, int format) {
    if (!pix || !width || !height || !bit_depth || !color_type || !raw) return false;
    if (!png_format_ok(c, format)) return false;
    const int px = png_expand_bytes(format);
    int64_t total_rows = 0;
    for (int i = 0; i < n; i++) {
        bool ok = pix[i] && raw[i] && png_dims_ok(width[i], height[i]) && png_color_ok(color_type[i], bit_depth[i]) && ((uintptr_t)pix[i] & (uintptr_t)(px - 1)) == 0;
        if (ok) {
            const int ct = color_type[i], tl = trns_len && ct != 4 && ct != 6 ? trns_len[i] : 0;
            if (ct == 3) ok = plte && plte[i] && plte_entries && plte_entries[i] >= 1 && plte_entries[i] <= 256 && tl >= 0 && tl <= plte_entries[i];
            else ok = tl == 0 || (ct == 0 && tl == 2) || (ct == 2 && tl == 6);
            if (ok && tl > 0) ok = trns && trns[i];
        }
        if (!ok) {
            c->err = "stream error";
            return false;
        }
        total_rows += height[i];
    }
    return png_rows_ok(c, total_rows);  // (the grid is the row list)
}

// The images of one KX launch: descriptors, the flat row list, and one table per palette image.
struct PngExpandJob {
    std::vector<PngExpandImg> img;
    PngOffsets rows;
    std::vector<uint32_t> tables;
    double ms = 0;  // profiling: the launches
    void add(const void *in, void *out, int64_t w, int64_t h, int depth, int color, int format, const uint8_t *plte, int entries, const uint8_t *trns, int trns_len) {
        PngExpandImg im{(const uint8_t *)in, (uint8_t *)out, (int32_t)w, (int32_t)h, depth, color, format, 0, {0, 0, 0}, 0};
        if (color == 3) {
            im.pal_off = (int32_t)tables.size();
            tables.resize(tables.size() + kPngPalEntries);
            png_expand_table(plte, entries, trns, trns_len, tables.data() + im.pal_off);
        } else if (trns_len > 0 && (color == 0 || color == 2)) {
            for (int k = 0; k < (color == 0 ? 1 : 3); k++) im.key[k] = (uint16_t)(trns[2 * k] << 8 | trns[2 * k + 1]);
            im.has_key = 1;
        }
        img.push_back(im);
        rows.add(h);
    }
};

// KX over the job on `s` (png_run_list: one wait)
bool png_expand_run(zs_ctx *c, PngExpandJob &job, int format, hipStream_t s, bool *no_memory) {
    const int m = (int)job.img.size();
    const size_t b_img = sizeof(PngExpandImg) * (size_t)m, b_off = job.rows.bytes(true);
    return png_run_list(c, c->png[kBufPngXimg], {{job.img.data(), b_img}, {job.tables.data(), sizeof(uint32_t) * job.tables.size()}}, job.rows, 0, kExpandGrid, s,
                        no_memory, &job.ms, [&](dim3 grid, dim3 block, uint8_t *d, int64_t row0) {
                            const PngExpandImg *d_img = (const PngExpandImg *)d;
                            const int32_t *d_off = (const int32_t *)(d + b_img);
                            const uint32_t *d_tab = (const uint32_t *)(d + b_img + b_off);
                            if (format == ZS_PNG_FMT_RGBA16) hipLaunchKernelGGL(zs_png_expand_kernel<ZS_PNG_FMT_RGBA16>, grid, block, 0, s, d_img, d_off, d_tab, m, row0);
                            else hipLaunchKernelGGL(zs_png_expand_kernel<ZS_PNG_FMT_RGBA8>, grid, block, 0, s, d_img, d_off, d_tab, m, row0);
                        });
}
}  // namespace

extern "C" int zs_png_expand_batch_device(zs_ctx *c, int n, const void *const *in, const int64_t *width, const int64_t *height, const int *bit_depth,
                                          const int *color_type, const void *const *plte, const int *plte_entries, const void *const *trns, const int *trns_len,
                                          int format, void *const *out, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!png_rgba_args_ok(c, n, (const void *const *)out, in, width, height, bit_depth, color_type, plte, plte_entries, trns, trns_len, format)) return ZS_STREAM_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    PngExpandJob job;
    for (int i = 0; i < n; i++) {
        const int ct = color_type[i], tl = trns_len && ct != 4 && ct != 6 ? trns_len[i] : 0;
        job.add(in[i], out[i], width[i], height[i], bit_depth[i], ct, format, ct == 3 ? (const uint8_t *)plte[i] : nullptr, ct == 3 ? plte_entries[i] : 0,
                tl > 0 ? (const uint8_t *)trns[i] : nullptr, tl);
    }
    bool no_memory = false;
    if (!png_expand_run(c, job, format, s, &no_memory)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    png_set_stage(c, kStPngExpand, job.ms);
    return png_done(hip_stream, s);
}

// ------------------------------------------------------------------ the pack from RGBA (KG, zs_png.hip): pixels a caller holds -> raw scanlines
namespace {
constexpr PngGrid kPackGrid{kPngSlice, kPackRowsPerWg, 64};

// The images of one KG launch: descriptors, the flat row list, and one lookup table per palette image.
struct PngPackJob {
    std::vector<PngPackImg> img;
    PngOffsets rows;
    std::vector<uint32_t> tables;
    double ms = 0;  // profiling: the launches
    // share_table >= 0: a palette image takes the table at that offset, made for an earlier image with the same PLTE / tRNS
    void add(const void *in, void *out, int64_t w, int64_t h, int depth, int color, int format, const uint8_t *plte, int entries, const uint8_t *trns, int trns_len,
             int32_t share_table = -1) {
        PngPackImg im{(const uint8_t *)in, (uint8_t *)out, (int32_t)w, (int32_t)h, depth, color, format, 0, {0, 0, 0}, 0};
        if (color == 3 && share_table >= 0) {
            im.pal_off = share_table;
        } else if (color == 3) {
            im.pal_off = (int32_t)tables.size();
            tables.resize(tables.size() + kPngPackTableWords);
            // (an entry at or beyond 2^depth has no index in the file: it cannot be named, and is left out)
            png_pack_table(plte, std::min(entries, 1 << depth), trns, trns_len, tables.data() + im.pal_off);
        } else if (trns_len > 0 && (color == 0 || color == 2)) {
            for (int k = 0; k < (color == 0 ? 1 : 3); k++) im.key[k] = (uint16_t)(trns[2 * k] << 8 | trns[2 * k + 1]);
            im.has_key = 1;
        }
        img.push_back(im);
        rows.add(h);
    }
};

// KG over the job on `s` (png_run_list: one wait), a zeroed word per image behind the tables for the palette pixels without an
// entry; and one more wait, for those counts, where `unmatched` is given.
bool png_pack_run(zs_ctx *c, PngPackJob &job, int format, int64_t *unmatched, hipStream_t s, bool *no_memory) {
    const int m = (int)job.img.size();
    const size_t b_img = sizeof(PngPackImg) * (size_t)m, b_off = job.rows.bytes(true), b_tab = sizeof(uint32_t) * job.tables.size(), b_cnt = sizeof(uint64_t) * (size_t)m;
    auto counts = [&](uint8_t *d) { return (unsigned long long *)(d + b_img + b_off + b_tab); };  // (8-aligned: every part in front is a multiple of 8)
    if (!png_run_list(c, c->png[kBufPngGimg], {{job.img.data(), b_img}, {job.tables.data(), b_tab}}, job.rows, b_cnt, kPackGrid, s, no_memory, &job.ms,
                      [&](dim3 grid, dim3 block, uint8_t *d, int64_t row0) {
                          const PngPackImg *d_img = (const PngPackImg *)d;
                          const int32_t *d_off = (const int32_t *)(d + b_img);
                          const uint32_t *d_tab = (const uint32_t *)(d + b_img + b_off);
                          if (format == ZS_PNG_FMT_RGBA16) hipLaunchKernelGGL(zs_png_pack_kernel<ZS_PNG_FMT_RGBA16>, grid, block, 0, s, d_img, d_off, d_tab, counts(d), m, row0);
                          else hipLaunchKernelGGL(zs_png_pack_kernel<ZS_PNG_FMT_RGBA8>, grid, block, 0, s, d_img, d_off, d_tab, counts(d), m, row0);
                      }))
        return false;
    if (unmatched) {
        ZS_HIP(c, hipMemcpyAsync(c->pinned, counts((uint8_t *)c->png[kBufPngGimg].p), b_cnt, hipMemcpyDeviceToHost, s));
        ZS_HIP(c, hipStreamSynchronize(s));
        memcpy(unmatched, c->pinned, b_cnt);
    }
    return true;
}
}  // namespace

extern "C" int zs_png_pack_batch_device(zs_ctx *c, int n, const void *const *in, const int64_t *width, const int64_t *height, const int *bit_depth,
                                        const int *color_type, const void *const *plte, const int *plte_entries, const void *const *trns, const int *trns_len,
                                        int format, void *const *out, int64_t *unmatched, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!png_rgba_args_ok(c, n, in, (const void *const *)out, width, height, bit_depth, color_type, plte, plte_entries, trns, trns_len, format)) return ZS_STREAM_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    PngPackJob job;
    for (int i = 0; i < n; i++) {
        const int ct = color_type[i], tl = trns_len && ct != 4 && ct != 6 ? trns_len[i] : 0;
        job.add(in[i], out[i], width[i], height[i], bit_depth[i], ct, format, ct == 3 ? (const uint8_t *)plte[i] : nullptr, ct == 3 ? plte_entries[i] : 0,
                tl > 0 ? (const uint8_t *)trns[i] : nullptr, tl);
    }
    bool no_memory = false;
    if (!png_pack_run(c, job, format, unmatched, s, &no_memory)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    png_set_stage(c, kStPngPack, job.ms);
    return png_done(hip_stream, s);
}

// ------------------------------------------------------------------ the survey (KV, zs_png.hip): what an image's pixels allow
extern "C" int zs_png_survey_batch_device(zs_ctx *c, int n, const void *const *in, const int64_t *width, const int64_t *height, int format, zs_png_survey *out,
                                          void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!in || !width || !height || !out) return ZS_STREAM_ERROR;
    if (!png_format_ok(c, format)) return ZS_STREAM_ERROR;
    const int px = png_expand_bytes(format);
    int64_t items = 0;
    for (int i = 0; i < n; i++) {
        if (!in[i] || !png_dims_ok(width[i], height[i]) || ((uintptr_t)in[i] & (uintptr_t)(px - 1)) != 0) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        items += (height[i] + kSurveyRows - 1) / kSurveyRows;
    }
    if (!png_rows_ok(c, items)) return ZS_STREAM_ERROR;  // (the first grid is the item list)
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const size_t b_img = sizeof(PngSurveyImg) * (size_t)n, b_off = sizeof(int32_t) * ((size_t)n + 1), b_res = sizeof(PngSurveyRec) * (size_t)n;
    // the records: the images' n in front, the items' behind them
    if (!ensure(c, c->png[kBufPngVimg], b_img + b_off) || !ensure(c, c->png[kBufPngVrec], sizeof(PngSurveyRec) * ((size_t)n + (size_t)items)) || !ensure_pinned(c, std::max(b_img + b_off, b_res)))
        return ZS_MEM_ERROR;
    {
        PngSurveyImg *h_img = (PngSurveyImg *)c->pinned;
        int32_t *h_off = (int32_t *)((uint8_t *)c->pinned + b_img);
        int64_t at = 0;
        for (int i = 0; i < n; i++) {
            h_img[i] = PngSurveyImg{(const uint8_t *)in[i], width[i], (int32_t)height[i], 0};
            h_off[i] = (int32_t)at;
            at += (height[i] + kSurveyRows - 1) / kSurveyRows;
        }
        h_off[n] = (int32_t)at;
    }
    auto hip_ok = [&](hipError_t e, const char *what) { return e == hipSuccess || fail(c, what, e); };
    if (!hip_ok(hipMemcpyAsync(c->png[kBufPngVimg].p, c->pinned, b_img + b_off, hipMemcpyHostToDevice, s), "hipMemcpyAsync")) return ZS_STREAM_ERROR;
    const bool prof = c->profiling;
    if (prof) (void)hipEventRecord(c->ev_png[0], s);
    const PngSurveyImg *d_img = (const PngSurveyImg *)c->png[kBufPngVimg].p;
    const int32_t *d_off = (const int32_t *)((const uint8_t *)c->png[kBufPngVimg].p + b_img);
    PngSurveyRec *d_res = (PngSurveyRec *)c->png[kBufPngVrec].p, *d_rec = d_res + n;
    if (format == ZS_PNG_FMT_RGBA16) hipLaunchKernelGGL(zs_png_survey_kernel<ZS_PNG_FMT_RGBA16>, dim3((unsigned)items), dim3(256), 0, s, d_img, d_off, n, d_rec);
    else hipLaunchKernelGGL(zs_png_survey_kernel<ZS_PNG_FMT_RGBA8>, dim3((unsigned)items), dim3(256), 0, s, d_img, d_off, n, d_rec);
    if (!hip_ok(hipGetLastError(), "zs_png_survey_kernel")) return ZS_STREAM_ERROR;
    hipLaunchKernelGGL(zs_png_survey_merge_kernel, dim3((unsigned)n), dim3(256), 0, s, d_off, d_rec, d_res);
    if (!hip_ok(hipGetLastError(), "zs_png_survey_merge_kernel")) return ZS_STREAM_ERROR;
    if (prof) (void)hipEventRecord(c->ev_png[1], s);
    // the one wait for the upload: the staging buffer is written again only by the copy behind it on the same stream
    if (!hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize")) return ZS_STREAM_ERROR;
    if (!hip_ok(hipMemcpyAsync(c->pinned, d_res, b_res, hipMemcpyDeviceToHost, s), "hipMemcpyAsync") || !hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize"))
        return ZS_STREAM_ERROR;
    if (prof) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->ev_png[0], c->ev_png[1]);
        png_set_stage(c, kStPngSurvey, ms);
    }
    const PngSurveyRec *res = (const PngSurveyRec *)c->pinned;
    for (int i = 0; i < n; i++) {
        const PngSurveyRec &r = res[i];
        zs_png_survey &o = out[i];
        memset(&o, 0, sizeof o);
        o.opaque = !(r.mask & kSvNotOpaque), o.gray = !(r.mask & kSvNotGray), o.low8 = !(r.mask & kSvNotLow8);
        o.sample_depth = !o.low8 ? 16 : (r.mask & kSvNot17) ? 8 : (r.mask & kSvNot85) ? 4 : (r.mask & kSvNot255) ? 2 : 1;
        const uint32_t white = (r.mask & kSvWhite) ? 1 : 0;
        o.n_colors = !o.low8 || r.count == kSurveyMany || r.count + white > 256 ? (int)kSurveyMany : (int)(r.count + white);
        if (o.n_colors > 256) continue;
        uint32_t key[256];  // A, R, G, B from the top byte down: ascending keys are the order asked for
        for (uint32_t k = 0; k < r.count; k++) key[k] = (r.colors[k] >> 24) << 24 | (r.colors[k] & 255) << 16 | (r.colors[k] >> 8 & 255) << 8 | (r.colors[k] >> 16 & 255);
        if (white) key[r.count] = 0xFFFFFFFFu;
        std::sort(key, key + o.n_colors);
        for (int k = 0; k < o.n_colors; k++)
            o.colors[k][0] = (uint8_t)(key[k] >> 16), o.colors[k][1] = (uint8_t)(key[k] >> 8), o.colors[k][2] = (uint8_t)key[k], o.colors[k][3] = (uint8_t)(key[k] >> 24);
    }
    return ZS_OK;
}

extern "C" int zs_png_choose_format(const zs_png_survey *sv, int *color_type, int *bit_depth) {
    if (!sv || !color_type || !bit_depth) return ZS_STREAM_ERROR;
    const int d = sv->sample_depth;
    if ((d != 1 && d != 2 && d != 4 && d != 8 && d != 16) || (d == 16) != !sv->low8 || sv->n_colors < 1 || sv->n_colors > 257) return ZS_STREAM_ERROR;
    png_choose_format(sv->opaque != 0, sv->gray != 0, sv->low8 != 0, d, sv->n_colors, color_type, bit_depth);
    return ZS_OK;
}

// ------------------------------------------------------------------ the Adam7 split (KS, zs_png.hip) and the interlaced encode call: pixels -> IDAT payloads
namespace {
constexpr PngGrid kSplitGrid{kPngSlice, kSplitRowsPerWg, 64};

// The images of one KS launch: descriptors and the flat list of pass rows.
struct PngSplitJob {
    std::vector<Adam7SplitImg> img;
    PngOffsets rows;
    double ms = 0;  // profiling: the launches
    void add(const void *pixels, void *passes, int64_t w, int64_t h, int bits) {
        Adam7SplitImg im{(const uint8_t *)pixels, (uint8_t *)passes, {}, {}, (int32_t)w, (int32_t)h, bits, 0};
        adam7_split_layout(im);
        img.push_back(im);
        rows.add(im.row0[kAdam7Passes]);
    }
};

// KS over the job on `s` (png_run_list: one wait)
bool png_split_run(zs_ctx *c, PngSplitJob &job, hipStream_t s, bool *no_memory) {
    static const int group = getenv("ZS_PNG_SPLIT_GROUP") ? atoi(getenv("ZS_PNG_SPLIT_GROUP")) : 8;  // (measurements: DESIGN.md section 4, KS)
    const int m = (int)job.img.size();
    const size_t b_img = sizeof(Adam7SplitImg) * (size_t)m;
    return png_run_list(c, c->png[kBufPngSimg], {{job.img.data(), b_img}}, job.rows, 0, kSplitGrid, s, no_memory, &job.ms,
                        [&](dim3 grid, dim3 block, uint8_t *d, int64_t row0) {
                            const Adam7SplitImg *d_img = (const Adam7SplitImg *)d;
                            const int32_t *d_off = (const int32_t *)(d + b_img);
                            if (group == 4) hipLaunchKernelGGL(zs_png_split_kernel<4>, grid, block, 0, s, d_img, d_off, m, row0);
                            else if (group == 16) hipLaunchKernelGGL(zs_png_split_kernel<16>, grid, block, 0, s, d_img, d_off, m, row0);
                            else hipLaunchKernelGGL(zs_png_split_kernel<8>, grid, block, 0, s, d_img, d_off, m, row0);
                        });
}
}  // namespace

extern "C" int zs_png_adam7_split_batch_device(zs_ctx *c, int n, const void *const *pixels, const int64_t *width, const int64_t *height,
                                               const int *bits_per_pixel, void *const *passes_out, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!pixels || !width || !height || !bits_per_pixel || !passes_out) {
        c->err = "stream error: a null array";
        return ZS_STREAM_ERROR;
    }
    int64_t total_rows = 0;
    for (int i = 0; i < n; i++) {
        if (!pixels[i] || !passes_out[i] || !png_dims_ok(width[i], height[i]) || !png_bits_ok(bits_per_pixel[i])) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        total_rows += adam7_pass_rows(width[i], height[i]);
    }
    if (!png_rows_ok(c, total_rows)) return ZS_STREAM_ERROR;  // (the grid is the list of pass rows)
    if (hipSetDevice(c->device) != hipSuccess) {
        c->err = "stream error: the context's device cannot be selected";
        return ZS_STREAM_ERROR;
    }
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    PngSplitJob job;
    for (int i = 0; i < n; i++) job.add(pixels[i], passes_out[i], width[i], height[i], bits_per_pixel[i]);
    bool no_memory = false;
    if (!png_split_run(c, job, s, &no_memory)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    png_set_stage(c, kStPngSplit, job.ms);
    if (hip_stream) return ZS_OK;
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) fail(c, "hipStreamSynchronize(s)", e);
    return e == hipSuccess ? ZS_OK : ZS_STREAM_ERROR;
}

// Pixels -> IDAT payloads, interlaced images among them: KS into a buffer of the context, the batch filter over every image
// and every present pass as an image of its own (the row above a pass's first row is zero: PNG specification 9.2), its outputs
// back to back, so that an image's filtered passes are one payload; then every image's rows -- pass rows in stream order -- as
// the Writes of its own stream.  Nothing leaves the device in between.
extern "C" int zs_png_idat_interlace_batch_device(zs_ctx *c, int n, const void *const *pixels, const int64_t *width, const int64_t *height,
                                                  const int *bits_per_pixel, const int *interlace, const int *filter, int64_t rows_per_write, void *const *out,
                                                  const int64_t *out_cap, int64_t *out_len, int *status, int level, int strategy, int hash_variant,
                                                  void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!pixels || !width || !height || !bits_per_pixel || !filter || !out || !out_cap || !out_len || rows_per_write < 0) return ZS_STREAM_ERROR;
    std::vector<int64_t> rb((size_t)n), len((size_t)n);
    std::vector<int> bpp((size_t)n);
    int64_t total_rows = 0, split_bytes = 0;
    int n_il = 0;
    size_t n_items = 0;
    for (int i = 0; i < n; i++) {
        const int il = interlace ? interlace[i] : 0;
        if (!pixels[i] || !out[i] || out_cap[i] < 0 || !png_dims_ok(width[i], height[i]) || !png_bits_ok(bits_per_pixel[i]) || (il != 0 && il != 1) || filter[i] < 0 ||
            filter[i] > 5) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        rb[(size_t)i] = png_bits_row_bytes(width[i], bits_per_pixel[i]);
        bpp[(size_t)i] = png_bits_bpp(bits_per_pixel[i]);
        len[(size_t)i] = zs_png_idat_layout(width[i], height[i], bits_per_pixel[i], il, nullptr, nullptr);
        if (len[(size_t)i] > 0x7FFFFFFF - 1024) {  // (a stream's input is indexed with 32 bits)
            c->err = "stream error: a filtered image is above 2 GiB - 1 KiB";
            return ZS_STREAM_ERROR;
        }
        const int64_t rows = il ? adam7_pass_rows(width[i], height[i]) : height[i];
        total_rows += rows;
        if (il) n_il++, split_bytes += ((len[(size_t)i] - rows) + 255) & ~(int64_t)255;
        for (int p = 0; p < kAdam7Passes; p++) n_items += il ? (adam7_pass_width(width[i], p) > 0 && adam7_pass_height(height[i], p) > 0) : p == 0;
    }
    if (!png_rows_ok(c, total_rows)) return ZS_STREAM_ERROR;  // (the grids are the row lists)
    // no interlaced image: the call is zs_png_idat_batch_device's, byte for byte and status for status
    if (n_il == 0)
        return zs_png_idat_batch_device(c, n, pixels, rb.data(), height, bpp.data(), filter, rows_per_write, out, out_cap, out_len, status, level, strategy,
                                        hash_variant, hip_stream);
    if (!check_args(c, n, len.data(), level, strategy)) return ZS_STREAM_ERROR;
    for (int i = 0; i < n; i++) {
        out_len[i] = 0;
        if (status) status[i] = ZS_STREAM_ERROR;
    }
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    size_t total = 0;
    for (int i = 0; i < n; i++) total += ((size_t)len[(size_t)i] + 255) & ~(size_t)255;
    if (!ensure(c, c->png[kBufPngScratch], total + 256) || !ensure(c, c->png[kBufPngSplit], (size_t)split_bytes + 256)) return ZS_MEM_ERROR;
    // ---- KS over the interlaced images
    PngSplitJob job;
    {
        int64_t at = 0;
        for (int i = 0; i < n; i++) {
            if (!(interlace && interlace[i])) continue;
            job.add(pixels[i], (uint8_t *)c->png[kBufPngSplit].p + at, width[i], height[i], bits_per_pixel[i]);
            at += ((len[(size_t)i] - job.img.back().row0[kAdam7Passes]) + 255) & ~(int64_t)255;
        }
    }
    bool no_memory = false;
    if (!png_split_run(c, job, s, &no_memory)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    // ---- the filter's items (an image, or a present pass), and every image's Write ends: rows of the stream in stream order
    std::vector<const void *> f_in(n_items);
    std::vector<void *> f_out(n_items);
    std::vector<int64_t> f_rb(n_items), f_h(n_items);
    std::vector<int> f_bpp(n_items), f_filter(n_items);
    std::vector<const void *> rows_in((size_t)n);
    std::vector<std::vector<int64_t>> ends((size_t)n);
    std::vector<const int64_t *> ends_p((size_t)n, nullptr);
    std::vector<int64_t> n_ends((size_t)n, 0);
    size_t at = 0, k = 0, j = 0;
    for (int i = 0; i < n; i++) {
        uint8_t *payload = (uint8_t *)c->png[kBufPngScratch].p + at;
        rows_in[(size_t)i] = payload;
        at += ((size_t)len[(size_t)i] + 255) & ~(size_t)255;
        const bool il = interlace && interlace[i];
        const Adam7SplitImg *sp = il ? &job.img[j++] : nullptr;
        int64_t pos = 0, row = 0;  // where the stream stands: bytes and rows
        const int64_t all_rows = il ? sp->row0[kAdam7Passes] : height[i];
        const bool cut = rows_per_write > 0 && rows_per_write < all_rows;
        for (int p = 0; p < (il ? kAdam7Passes : 1); p++) {
            const int64_t pw = il ? adam7_pass_width(width[i], p) : width[i], ph = il ? adam7_pass_height(height[i], p) : height[i];
            if (pw <= 0 || ph <= 0) continue;
            const int64_t prb = png_bits_row_bytes(pw, bits_per_pixel[i]);
            f_in[k] = il ? (const void *)(sp->passes + sp->off[p]) : pixels[i];
            f_out[k] = payload + pos;
            f_rb[k] = prb, f_h[k] = ph, f_bpp[k] = bpp[(size_t)i], f_filter[k] = filter[i];
            k++;
            if (cut) {
                // the Write ends inside this pass: after stream rows rows_per_write, 2 * rows_per_write, ...
                int64_t r = (row / rows_per_write + 1) * rows_per_write;  // the first multiple above `row`
                for (; r <= row + ph && r < all_rows; r += rows_per_write) ends[(size_t)i].push_back(pos + (r - row) * (prb + 1));
            }
            pos += ph * (prb + 1), row += ph;
        }
        if (cut) {
            ends[(size_t)i].push_back(len[(size_t)i]);
            ends_p[(size_t)i] = ends[(size_t)i].data(), n_ends[(size_t)i] = (int64_t)ends[(size_t)i].size();
        }
    }
    if (!run_png_filter_batch(c, (int)n_items, f_in.data(), f_rb.data(), f_h.data(), f_bpp.data(), f_filter.data(), f_out.data(), s)) return ZS_STREAM_ERROR;
    const int rc = zs_deflate_writes_batch_device(c, n, rows_in.data(), len.data(), ends_p.data(), n_ends.data(), out, out_cap, out_len, status, level, strategy,
                                                  hash_variant, hip_stream);
    if (c->profiling) c->stage_ms[kStPngSplit] = job.ms;
    return rc;
}

// ------------------------------------------------------------------ CRC-32 (KC, zs_crc32.hip), PNG files on top of it
namespace {
static_assert(sizeof(zs_png_info) == sizeof(PngFileInfo) && offsetof(zs_png_info, n_idat) == offsetof(PngFileInfo, n_idat), "zs_png_info mirrors PngFileInfo");

// One KC job: m spans and `blob` bytes the caller's spans may read or frame (host bytes that travel with the descriptors),
// laid out in the staging buffer as [spans][tile offsets][blob][results] and on the device, in png[kBufCrcDesc], as the first three.
struct Crc32Job {
    int m = 0;
    size_t b_sp = 0, b_off = 0, b_blob = 0;
    Crc32Span *spans = nullptr;     // staging: the caller fills these ...
    uint8_t *blob = nullptr;        // ... and this,
    uint8_t *d_blob = nullptr;      // which the device sees here
    const uint32_t *crc = nullptr;  // staging: zlib's crc32 of every span, once the job has run
    double ms = 0;                  // profiling: KC and its finishing launch
};

bool crc32_begin(zs_ctx *c, int m, size_t blob_bytes, Crc32Job *job, bool *no_memory) {
    *no_memory = false;
    if (!c->crc32_tab) {
        std::vector<uint32_t> tab((size_t)kCrcTabWords);
        crc32_fill_tables(tab.data());
        if (hipMalloc((void **)&c->crc32_tab, 4 * tab.size()) != hipSuccess) {
            (void)hipGetLastError();
            c->crc32_tab = nullptr;
            c->err = "out of device memory";
            *no_memory = true;
            return false;
        }
        ZS_HIP(c, hipMemcpy(c->crc32_tab, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice));
    }
    job->m = m;
    job->b_sp = sizeof(Crc32Span) * (size_t)m;
    job->b_off = (sizeof(uint32_t) * ((size_t)m + 1) + 255) & ~(size_t)255;
    job->b_blob = (blob_bytes + 255) & ~(size_t)255;
    const size_t up = job->b_sp + job->b_off + job->b_blob;
    if (!ensure(c, c->png[kBufCrcDesc], up) || !ensure(c, c->png[kBufCrcRes], 2 * sizeof(uint32_t) * (size_t)m) || !ensure_pinned(c, up + sizeof(uint32_t) * (size_t)m)) {
        *no_memory = true;
        return false;
    }
    uint8_t *hp = (uint8_t *)c->pinned;
    job->spans = (Crc32Span *)hp;
    job->blob = hp + job->b_sp + job->b_off;
    job->d_blob = (uint8_t *)c->png[kBufCrcDesc].p + job->b_sp + job->b_off;
    job->crc = (const uint32_t *)(hp + up);
    return true;
}

// Uploads the job, runs KC and the finishing launch and waits for `s` once; the CRCs are in job->crc afterwards.
// behind (may be null): work the caller puts on `s` behind the finishing launch and in front of that one wait -- it is given
// the CRCs' place on the device (a gzip trailer is written from there, zs_wrap_host.inc); false from it fails the job.
bool crc32_run(zs_ctx *c, Crc32Job *job, hipStream_t s, const std::function<bool(const uint32_t *)> *behind = nullptr) {
    const int m = job->m;
    uint32_t *off = (uint32_t *)((uint8_t *)c->pinned + job->b_sp);
    uint64_t tiles = 0;
    for (int i = 0; i < m; i++) {
        off[i] = (uint32_t)tiles;
        tiles += (uint64_t)crc32_span_tiles(job->spans[i].len);
        if (tiles > 0x7FFFFFFFu) {
            c->err = "stream error: more than 2^31 - 1 tiles of 8 KiB in one call (split the batch)";
            return false;
        }
    }
    off[m] = (uint32_t)tiles;
    const size_t up = job->b_sp + job->b_off + job->b_blob;
    const Crc32Span *d_sp = (const Crc32Span *)c->png[kBufCrcDesc].p;
    const uint32_t *d_off = (const uint32_t *)((const uint8_t *)c->png[kBufCrcDesc].p + job->b_sp);
    uint32_t *d_res = (uint32_t *)c->png[kBufCrcRes].p, *d_crc = d_res + m;
    ZS_HIP(c, hipMemcpyAsync(c->png[kBufCrcDesc].p, c->pinned, up, hipMemcpyHostToDevice, s));
    const bool prof = c->profiling;
    if (prof) (void)hipEventRecord(c->ev_png[0], s);
    ZS_HIP(c, hipMemsetAsync(d_res, 0, sizeof(uint32_t) * (size_t)m, s));
    if (tiles) {
        // (measurements of the two forms: DESIGN.md section 4, KC)
        static const int form = getenv("ZS_CRC32_FORM") ? atoi(getenv("ZS_CRC32_FORM")) : 0;
        const unsigned groups = (unsigned)((tiles + kCrcWaves - 1) / kCrcWaves);
        const dim3 grid(std::min<unsigned>(groups, 2048)), block(64 * kCrcWaves);  // eight workgroups a CU keep their tables
        if (form == 1) hipLaunchKernelGGL(zs_crc32_tile_kernel<false>, grid, block, 0, s, d_sp, d_off, m, (uint32_t)tiles, c->crc32_tab, d_res);
        else hipLaunchKernelGGL(zs_crc32_tile_kernel<true>, grid, block, 0, s, d_sp, d_off, m, (uint32_t)tiles, c->crc32_tab, d_res);
        ZS_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(zs_crc32_finish_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, d_sp, m, (const uint32_t *)d_res, d_crc);
    ZS_HIP(c, hipGetLastError());
    if (behind && !(*behind)(d_crc)) return false;
    if (prof) (void)hipEventRecord(c->ev_png[1], s);
    ZS_HIP(c, hipMemcpyAsync((void *)job->crc, d_crc, sizeof(uint32_t) * (size_t)m, hipMemcpyDeviceToHost, s));
    ZS_HIP(c, hipStreamSynchronize(s));
    if (prof) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->ev_png[0], c->ev_png[1]);
        job->ms = ms;
    }
    return true;
}
constexpr int64_t kCrcMaxLen = 0x7FFFFFFF - 1024;
}  // namespace

extern "C" int zs_crc32_batch_device(zs_ctx *c, int n, const void *const *d_buf, const int64_t *len, const uint32_t *seed, uint32_t *out, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!d_buf || !len || !out) return ZS_STREAM_ERROR;
    for (int i = 0; i < n; i++)
        if (len[i] < 0 || len[i] > kCrcMaxLen || (len[i] > 0 && !d_buf[i])) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    Crc32Job job;
    bool no_memory = false;
    if (!crc32_begin(c, n, 0, &job, &no_memory)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    for (int i = 0; i < n; i++) job.spans[i] = Crc32Span{(const uint8_t *)d_buf[i], nullptr, nullptr, len[i], ~(seed ? seed[i] : 0u), 0, 0, 0};
    if (!crc32_run(c, &job, s)) return ZS_STREAM_ERROR;
    memcpy(out, job.crc, sizeof(uint32_t) * (size_t)n);
    png_set_stage(c, kStCrc32, job.ms);
    return ZS_OK;
}

extern "C" int zs_crc32_device(zs_ctx *c, const void *d_buf, int64_t len, uint32_t seed, uint32_t *out, void *hip_stream) {
    return zs_crc32_batch_device(c, 1, &d_buf, &len, &seed, out, hip_stream);
}

extern "C" int64_t zs_png_file_bound(int64_t idat_len, int64_t idat_chunk_bytes, int64_t extra_len) {
    return png_file_bound(idat_len, idat_chunk_bytes, extra_len);
}

// Pixels -> files: the IDAT call into a buffer of the context, then KC over [signature, IHDR, extra] / every IDAT chunk / IEND
// of every image that fits its output.  interlace: null (zs_png_encode_batch_device) or IHDR's interlace byte per image; with
// no interlaced image the IDAT call, and so every byte and status, is zs_png_idat_batch_device's.
namespace {
int png_encode_files(zs_ctx *c, int n, const void *const *pixels, const int64_t *width, const int64_t *height, const int *bit_depth, const int *color_type,
                     const int *filter, const int *interlace, const void *const *extra, const int64_t *extra_len, int64_t rows_per_write,
                     int64_t idat_chunk_bytes, void *const *out, const int64_t *out_cap, int64_t *out_len, int *status, int level, int strategy,
                     int hash_variant, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!pixels || !width || !height || !bit_depth || !color_type || !filter || !out || !out_cap || !out_len || (extra && !extra_len)) return ZS_STREAM_ERROR;
    if (rows_per_write < 0 || idat_chunk_bytes < 0 || idat_chunk_bytes > kPngMaxChunk || level < -1 || level > 9 || strategy < 0 || strategy > 4) {
        c->err = "stream error";
        return ZS_STREAM_ERROR;
    }
    std::vector<int64_t> rb((size_t)n), xlen((size_t)n, 0), zcap((size_t)n);
    std::vector<int> bpp((size_t)n), bits_pp((size_t)n);
    int64_t total_rows = 0;
    size_t z_total = 0, x_total = 0;
    bool any_interlaced = false;
    for (int i = 0; i < n; i++) {
        const int il = interlace ? interlace[i] : 0;
        if (il != 0 && il != 1) {
            c->err = "stream error: interlace is neither 0 nor 1";
            return ZS_STREAM_ERROR;
        }
        if (!pixels[i] || !out[i] || !png_dims_ok(width[i], height[i]) || !png_color_ok(color_type[i], bit_depth[i]) || filter[i] < 0 || filter[i] > 5 || out_cap[i] < 0) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        const int bits = bit_depth[i] * png_channels(color_type[i]);
        rb[(size_t)i] = png_bits_row_bytes(width[i], bits);
        bpp[(size_t)i] = png_bits_bpp(bits);
        bits_pp[(size_t)i] = bits;
        any_interlaced = any_interlaced || il;
        // the filtered image: the rows, or the present passes' rows, each with its filter byte
        const int64_t filtered = il ? zs_png_idat_layout(width[i], height[i], bits, 1, nullptr, nullptr) : height[i] * (rb[(size_t)i] + 1);
        if (filtered > kCrcMaxLen) {  // (a stream's input is indexed with 32 bits)
            c->err = "stream error: a filtered image is above 2 GiB - 1 KiB";
            return ZS_STREAM_ERROR;
        }
        if (extra) {
            xlen[(size_t)i] = extra_len[i];
            if (xlen[(size_t)i] < 0 || (xlen[(size_t)i] > 0 && !extra[i]) || !png_chunks_well_formed((const uint8_t *)extra[i], xlen[(size_t)i])) {
                c->err = "stream error: the extra chunks of an image are not a sequence of whole chunks";
                return ZS_STREAM_ERROR;
            }
        }
        zcap[(size_t)i] = zs_deflate_bound(filtered);
        z_total += ((size_t)zcap[(size_t)i] + 255) & ~(size_t)255;
        x_total += 8 + 25 + (size_t)xlen[(size_t)i] + 12;
        total_rows += il ? adam7_pass_rows(width[i], height[i]) : height[i];
    }
    if (!png_rows_ok(c, total_rows)) return ZS_STREAM_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    std::vector<int> st((size_t)n, ZS_STREAM_ERROR);
    auto finish = [&](int rc) {
        if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
        return rc;
    };
    if (!ensure(c, c->png[kBufPngZs], z_total + 256)) {
        std::fill(st.begin(), st.end(), (int)ZS_MEM_ERROR);
        return finish(ZS_MEM_ERROR);
    }
    std::vector<void *> zs_out((size_t)n);
    std::vector<int64_t> zlen((size_t)n, 0);
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        zs_out[(size_t)i] = (uint8_t *)c->png[kBufPngZs].p + at;
        at += ((size_t)zcap[(size_t)i] + 255) & ~(size_t)255;
    }
    const int zrc = any_interlaced ? zs_png_idat_interlace_batch_device(c, n, pixels, width, height, bits_pp.data(), interlace, filter, rows_per_write, zs_out.data(),
                                                                        zcap.data(), zlen.data(), st.data(), level, strategy, hash_variant, (void *)s)
                                   : zs_png_idat_batch_device(c, n, pixels, rb.data(), height, bpp.data(), filter, rows_per_write, zs_out.data(), zcap.data(),
                                                              zlen.data(), st.data(), level, strategy, hash_variant, (void *)s);
    if (zrc != ZS_OK) {
        for (int i = 0; i < n; i++) out_len[i] = 0;
        return finish(zrc);
    }
    // ---- the layout: which images fit, and their spans
    int64_t n_spans = 0;
    int rc = ZS_OK;
    for (int i = 0; i < n; i++) {
        out_len[i] = png_file_bound(zlen[(size_t)i], idat_chunk_bytes, xlen[(size_t)i]);
        if (out_len[i] < 0) {  // (one chunk cannot hold the stream: unreachable below 2 GiB)
            st[(size_t)i] = ZS_STREAM_ERROR;
            if (rc == ZS_OK) rc = ZS_STREAM_ERROR, c->err = "stream error";
            continue;
        }
        if (out_cap[i] < out_len[i]) {
            st[(size_t)i] = ZS_BUF_ERROR;
            if (rc == ZS_OK) rc = ZS_BUF_ERROR, c->err = "buffer error";
            continue;
        }
        const int64_t chunks = idat_chunk_bytes == 0 || zlen[(size_t)i] == 0 ? 1 : (zlen[(size_t)i] + idat_chunk_bytes - 1) / idat_chunk_bytes;
        n_spans += 2 + chunks;
    }
    if (n_spans > 0x3FFFFFFF) {
        c->err = "stream error: too many IDAT chunks in one call";
        return finish(ZS_STREAM_ERROR);
    }
    if (n_spans == 0) return finish(rc);
    Crc32Job job;
    bool no_memory = false;
    if (!crc32_begin(c, (int)n_spans, x_total, &job, &no_memory)) {
        for (int i = 0; i < n; i++)
            if (st[(size_t)i] == ZS_OK) st[(size_t)i] = no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
        return finish(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    }
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    static const uint8_t idat_type[4] = {'I', 'D', 'A', 'T'};
    const uint32_t idat_init = ~crc32_bytes_slow(0, idat_type, 4);
    size_t k = 0, b = 0;
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        uint8_t *o = (uint8_t *)out[i];
        // signature, IHDR and the caller's chunks: host bytes, placed by a copy span
        uint8_t *hd = job.blob + b;
        memcpy(hd, sig, 8);
        png_put_be32(hd + 8, 13);
        memcpy(hd + 12, "IHDR", 4);
        png_put_be32(hd + 16, (uint32_t)width[i]), png_put_be32(hd + 20, (uint32_t)height[i]);
        hd[24] = (uint8_t)bit_depth[i], hd[25] = (uint8_t)color_type[i], hd[26] = 0, hd[27] = 0, hd[28] = (uint8_t)(interlace ? interlace[i] : 0);
        png_put_be32(hd + 29, crc32_bytes_slow(0, hd + 12, 17));
        if (xlen[(size_t)i]) memcpy(hd + 33, extra[i], (size_t)xlen[(size_t)i]);
        const int64_t head = 33 + xlen[(size_t)i];
        job.spans[k++] = Crc32Span{job.d_blob + b, o, nullptr, head, 0xFFFFFFFFu, 0, 0, 0};
        b += (size_t)head;
        int64_t pos = head, zat = 0;
        const int64_t zl = zlen[(size_t)i], step = idat_chunk_bytes == 0 ? zl : idat_chunk_bytes;
        do {
            const int64_t len = std::min(step, zl - zat);
            job.spans[k++] = Crc32Span{(const uint8_t *)zs_out[(size_t)i] + zat, o + pos + 8, o + pos, len, idat_init, 0, kPngIDAT, 0};
            pos += 12 + len, zat += len;
        } while (zat < zl);
        uint8_t *tl = job.blob + b;
        png_put_be32(tl, 0);
        memcpy(tl + 4, "IEND", 4);
        png_put_be32(tl + 8, crc32_bytes_slow(0, tl + 4, 4));
        job.spans[k++] = Crc32Span{job.d_blob + b, o + pos, nullptr, 12, 0xFFFFFFFFu, 0, 0, 0};
        b += 12;
    }
    if (!crc32_run(c, &job, s)) return finish(ZS_STREAM_ERROR);
    if (c->profiling) c->stage_ms[kStCrc32] = job.ms;
    return finish(rc);
}
}  // namespace

extern "C" int zs_png_encode_batch_device(zs_ctx *c, int n, const void *const *pixels, const int64_t *width, const int64_t *height, const int *bit_depth,
                                          const int *color_type, const int *filter, const void *const *extra, const int64_t *extra_len, int64_t rows_per_write,
                                          int64_t idat_chunk_bytes, void *const *out, const int64_t *out_cap, int64_t *out_len, int *status, int level,
                                          int strategy, int hash_variant, void *hip_stream) {
    return png_encode_files(c, n, pixels, width, height, bit_depth, color_type, filter, nullptr, extra, extra_len, rows_per_write, idat_chunk_bytes, out, out_cap,
                            out_len, status, level, strategy, hash_variant, hip_stream);
}

extern "C" int zs_png_encode_interlace_batch_device(zs_ctx *c, int n, const void *const *pixels, const int64_t *width, const int64_t *height,
                                                    const int *bit_depth, const int *color_type, const int *filter, const int *interlace,
                                                    const void *const *extra, const int64_t *extra_len, int64_t rows_per_write, int64_t idat_chunk_bytes,
                                                    void *const *out, const int64_t *out_cap, int64_t *out_len, int *status, int level, int strategy,
                                                    int hash_variant, void *hip_stream) {
    return png_encode_files(c, n, pixels, width, height, bit_depth, color_type, filter, interlace, extra, extra_len, rows_per_write, idat_chunk_bytes, out,
                            out_cap, out_len, status, level, strategy, hash_variant, hip_stream);
}

namespace {
// What the survey of an image (or of an animation's canvases) decides on the host: the pair, and for a palette image the PLTE
// in the survey's order and the tRNS up to the last entry below 255 (none when all are 255), framed behind the caller's
// chunks in `xs`.
struct PngChosen {
    int ct = 0, bd = 0, entries = 0, tlen = 0;
    std::vector<uint8_t> xs, plte, trns;
};
bool png_choose_chunks(const zs_png_survey &sv, const void *extra, int64_t extra_len, PngChosen *o) {
    auto put_chunk = [](std::vector<uint8_t> &to, const char *type, const std::vector<uint8_t> &data) {
        const size_t at = to.size();
        to.resize(at + 12 + data.size());
        png_put_be32(to.data() + at, (uint32_t)data.size());
        memcpy(to.data() + at + 4, type, 4);
        if (!data.empty()) memcpy(to.data() + at + 8, data.data(), data.size());
        png_put_be32(to.data() + at + 8 + data.size(), crc32_bytes_slow(0, to.data() + at + 4, (int64_t)(4 + data.size())));
    };
    if (zs_png_choose_format(&sv, &o->ct, &o->bd) != ZS_OK) return false;
    if (extra && extra_len > 0) o->xs.assign((const uint8_t *)extra, (const uint8_t *)extra + extra_len);
    if (o->ct != 3) return true;
    const int m = sv.n_colors;
    o->entries = m;
    o->plte.resize(3 * (size_t)m);
    for (int e = 0; e < m; e++) {
        memcpy(o->plte.data() + 3 * (size_t)e, sv.colors[e], 3);
        if (sv.colors[e][3] != 255) o->tlen = e + 1;
    }
    o->trns.resize((size_t)o->tlen);
    for (int e = 0; e < o->tlen; e++) o->trns[(size_t)e] = sv.colors[e][3];
    put_chunk(o->xs, "PLTE", o->plte);
    if (o->tlen > 0) put_chunk(o->xs, "tRNS", o->trns);
    return true;
}
}  // namespace

// RGBA pixels -> files: the survey (KV), the choice per image on the host, PLTE and tRNS of the palette images framed on the
// host behind the caller's chunks, the pack (KG) into a buffer of the context, then the body of the two calls above on that
// buffer.  Every argument is checked here first, so that nothing the later steps refuse has touched status by then.
extern "C" int zs_png_encode_rgba_batch_device(zs_ctx *c, int n, const void *const *pixels, const int64_t *width, const int64_t *height, int format,
                                               const int *filter, const int *interlace, const void *const *extra, const int64_t *extra_len,
                                               int64_t rows_per_write, int64_t idat_chunk_bytes, void *const *out, const int64_t *out_cap, int64_t *out_len,
                                               int *status, int *color_type_out, int *bit_depth_out, int level, int strategy, int hash_variant,
                                               void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!pixels || !width || !height || !filter || !out || !out_cap || !out_len || (extra && !extra_len)) return ZS_STREAM_ERROR;
    if (!png_format_ok(c, format)) return ZS_STREAM_ERROR;
    if (rows_per_write < 0 || idat_chunk_bytes < 0 || idat_chunk_bytes > kPngMaxChunk || level < -1 || level > 9 || strategy < 0 || strategy > 4) {
        c->err = "stream error";
        return ZS_STREAM_ERROR;
    }
    const int px = png_expand_bytes(format);
    int64_t total_rows = 0;
    for (int i = 0; i < n; i++) {
        const int il = interlace ? interlace[i] : 0;
        if (il != 0 && il != 1) {
            c->err = "stream error: interlace is neither 0 nor 1";
            return ZS_STREAM_ERROR;
        }
        if (!pixels[i] || !out[i] || !png_dims_ok(width[i], height[i]) || filter[i] < 0 || filter[i] > 5 || out_cap[i] < 0 || ((uintptr_t)pixels[i] & (uintptr_t)(px - 1)) != 0) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        // (the pair is not chosen yet: the limit is held against the pixels as they come, which no choice exceeds)
        if (width[i] * height[i] > kCrcMaxLen / px || zs_png_idat_layout(width[i], height[i], 8 * px, il, nullptr, nullptr) > kCrcMaxLen) {
            c->err = "stream error: a filtered image is above 2 GiB - 1 KiB";
            return ZS_STREAM_ERROR;
        }
        if (extra && (extra_len[i] < 0 || (extra_len[i] > 0 && !extra[i]) || !png_chunks_well_formed((const uint8_t *)extra[i], extra_len[i]))) {
            c->err = "stream error: the extra chunks of an image are not a sequence of whole chunks";
            return ZS_STREAM_ERROR;
        }
        total_rows += il ? adam7_pass_rows(width[i], height[i]) : height[i];
    }
    if (!png_rows_ok(c, total_rows)) return ZS_STREAM_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    auto all_fail = [&](int rc) {
        for (int i = 0; i < n; i++) {
            out_len[i] = 0;
            if (status) status[i] = rc;
        }
        return rc;
    };
    // ---- the survey and the choice
    std::vector<zs_png_survey> sv((size_t)n);
    int rc = zs_png_survey_batch_device(c, n, pixels, width, height, format, sv.data(), (void *)s);
    if (rc != ZS_OK) return all_fail(rc);
    const double survey_ms = c->profiling ? c->stage_ms[kStPngSurvey] : 0;
    std::vector<PngChosen> ch((size_t)n);
    std::vector<int> ct((size_t)n), bd((size_t)n);
    std::vector<const void *> x_ptr((size_t)n), packed((size_t)n);
    std::vector<int64_t> x_len((size_t)n);
    size_t pack_total = 0;
    for (int i = 0; i < n; i++) {
        const size_t k = (size_t)i;
        if (!png_choose_chunks(sv[k], extra ? extra[i] : nullptr, extra ? extra_len[i] : 0, &ch[k])) return all_fail(ZS_STREAM_ERROR);  // (unreachable: the survey is our own)
        ct[k] = ch[k].ct, bd[k] = ch[k].bd;
        if (color_type_out) color_type_out[i] = ct[k];
        if (bit_depth_out) bit_depth_out[i] = bd[k];
        x_ptr[k] = ch[k].xs.empty() ? nullptr : ch[k].xs.data();
        x_len[k] = (int64_t)ch[k].xs.size();
        pack_total += ((size_t)(png_bits_row_bytes(width[i], bd[k] * png_channels(ct[k])) * height[i]) + 255) & ~(size_t)255;
    }
    // ---- the pack
    if (!ensure(c, c->png[kBufPngPacked], pack_total + 256)) return all_fail(ZS_MEM_ERROR);
    PngPackJob job;
    {
        size_t at = 0;
        for (int i = 0; i < n; i++) {
            const size_t k = (size_t)i;
            packed[k] = (uint8_t *)c->png[kBufPngPacked].p + at;
            job.add(pixels[i], (void *)packed[k], width[i], height[i], bd[k], ct[k], format, ch[k].ct == 3 ? ch[k].plte.data() : nullptr, ch[k].entries,
                    ch[k].tlen > 0 ? ch[k].trns.data() : nullptr, ch[k].tlen);
            at += ((size_t)(png_bits_row_bytes(width[i], bd[k] * png_channels(ct[k])) * height[i]) + 255) & ~(size_t)255;
        }
    }
    bool no_memory = false;
    if (!png_pack_run(c, job, format, nullptr, s, &no_memory)) return all_fail(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    rc = png_encode_files(c, n, packed.data(), width, height, bd.data(), ct.data(), filter, interlace, x_ptr.data(), x_len.data(), rows_per_write, idat_chunk_bytes, out,
                          out_cap, out_len, status, level, strategy, hash_variant, hip_stream);
    if (c->profiling) c->stage_ms[kStPngSurvey] = survey_ms, c->stage_ms[kStPngPack] = job.ms;
    return rc;
}

extern "C" int zs_png_file_info(const void *file, int64_t len, zs_png_info *info) {
    if (!file || !info || len < 0) return ZS_STREAM_ERROR;
    char msg[160];
    return png_walk_file((const uint8_t *)file, len, (PngFileInfo *)info, msg, sizeof msg, true, [](const PngChunkRef &) {}) ? ZS_OK : ZS_DATA_ERROR;
}

extern "C" int zs_png_file_colors(const void *file, int64_t len, void *plte768, int *plte_entries, void *trns256, int *trns_len) {
    if (!file || len < 0 || !plte768 || !plte_entries || !trns256 || !trns_len) return ZS_STREAM_ERROR;
    char msg[160];
    PngFileInfo info;
    PngFileColors col;
    if (!png_walk_file((const uint8_t *)file, len, &info, msg, sizeof msg, true, [](const PngChunkRef &) {}) ||
        !png_file_colors((const uint8_t *)file, len, info, &col, msg, sizeof msg))
        return ZS_DATA_ERROR;
    memcpy(plte768, col.plte, 3 * (size_t)col.plte_entries), *plte_entries = col.plte_entries;
    memcpy(trns256, col.trns, (size_t)col.trns_len), *trns_len = col.trns_len;
    return ZS_OK;
}

namespace {
// Files -> pixels: the walk on the host, one upload, KC over the critical chunks (IDAT data gathered on the way), then the
// decode call on the gathered streams of the files that are whole.  format < 0: the raw scanlines go to out[i]; otherwise
// (zs_png_decode_files_rgba_batch) into a buffer of the context, and KX takes them from there to out[i] in that format.
int png_decode_files(zs_ctx *c, int n, const void *const *file, const int64_t *file_len, int format, void *const *out, const int64_t *out_cap,
                     zs_png_info *info, int *status, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!file || !file_len || !out || !out_cap) return ZS_STREAM_ERROR;
    const bool expand = format >= 0;
    if (expand && !png_format_ok(c, format)) return ZS_STREAM_ERROR;
    const int px = expand ? png_expand_bytes(format) : 1;
    for (int i = 0; i < n; i++)
        if (!file[i] || !out[i] || file_len[i] < 0 || out_cap[i] < 0 || ((uintptr_t)out[i] & (uintptr_t)(px - 1)) != 0) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
    std::vector<PngFileColors> colors(expand ? (size_t)n : 0);
    std::vector<int64_t> raw_at((size_t)n, 0);
    size_t raw_total = 0;
    std::vector<PngFileInfo> fi((size_t)n);
    std::vector<std::string> why((size_t)n);
    std::vector<int> st((size_t)n, ZS_OK);
    std::vector<std::vector<PngChunkRef>> refs((size_t)n);
    size_t blob = 0, gather = 0;
    int64_t n_spans = 0, rows = 0;
    char msg[192];
    for (int i = 0; i < n; i++) {
        auto &r = refs[(size_t)i];
        PngFileInfo &f = fi[(size_t)i];
        if (!png_walk_file((const uint8_t *)file[i], file_len[i], &f, msg, sizeof msg, false, [&](const PngChunkRef &x) { r.push_back(x); }) ||
            (expand && !png_file_colors((const uint8_t *)file[i], file_len[i], f, &colors[(size_t)i], msg, sizeof msg))) {
            st[(size_t)i] = ZS_DATA_ERROR, why[(size_t)i] = msg;
        } else if (f.idat_bytes > kCrcMaxLen || zs_png_idat_layout(f.width, f.height, f.bits_per_pixel, f.interlace, nullptr, nullptr) > kCrcMaxLen) {
            st[(size_t)i] = ZS_DATA_ERROR, why[(size_t)i] = "the image or its IDAT data is above 2 GiB - 1 KiB";
        } else if (out_cap[i] < (expand ? f.width * f.height * px : f.pixel_bytes)) {  // (an image below 2 GiB of scanlines has fewer than 2^34 pixels)
            snprintf(msg, sizeof msg, "the image needs %lld bytes, out_cap is %lld", (long long)(expand ? f.width * f.height * px : f.pixel_bytes), (long long)out_cap[i]);
            st[(size_t)i] = ZS_BUF_ERROR, why[(size_t)i] = msg;
        }
        if (info) memcpy(&info[i], &f, sizeof f);
        if (st[(size_t)i] != ZS_OK) continue;
        if (expand) raw_at[(size_t)i] = (int64_t)raw_total, raw_total += ((size_t)f.pixel_bytes + 255) & ~(size_t)255;
        int64_t r7[kAdam7Passes];
        (void)zs_png_idat_layout(f.width, f.height, f.bits_per_pixel, f.interlace, nullptr, r7);
        for (int64_t v : r7) rows += v;
        blob += ((size_t)file_len[i] + 255) & ~(size_t)255;
        gather += ((size_t)f.idat_bytes + 255) & ~(size_t)255;
        n_spans += (int64_t)r.size();
    }
    auto finish = [&](int rc) {
        if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
        return rc;
    };
    auto verdict = [&]() {  // the first failing file's code and message
        for (int i = 0; i < n; i++)
            if (st[(size_t)i] != ZS_OK) {
                c->err = std::string(st[(size_t)i] == ZS_BUF_ERROR ? "buffer error: file " : "data error: file ") + std::to_string(i) + ": " + why[(size_t)i];
                return finish(st[(size_t)i]);
            }
        return finish(ZS_OK);
    };
    if (n_spans > 0x3FFFFFFF || rows > 0x7FFFFFFF) {
        c->err = "stream error: too many chunks or rows in one call (split the batch)";
        return ZS_STREAM_ERROR;
    }
    if (n_spans == 0) return verdict();
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    auto all_fail = [&](int code) {
        for (int &v : st)
            if (v == ZS_OK) v = code;
        return finish(code);
    };
    Crc32Job job;
    bool no_memory = false;
    if (!ensure(c, c->png[kBufPngGather], gather + 256) || (expand && !ensure(c, c->png[kBufPngRaw], raw_total + 256))) return all_fail(ZS_MEM_ERROR);
    if (!crc32_begin(c, (int)n_spans, blob, &job, &no_memory)) return all_fail(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    std::vector<const void *> idat;
    std::vector<int> who;  // the files that go on
    size_t k = 0, b = 0, g = 0;
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        memcpy(job.blob + b, file[i], (size_t)file_len[i]);
        who.push_back(i);
        idat.push_back((const uint8_t *)c->png[kBufPngGather].p + g);
        size_t ga = g;
        for (const PngChunkRef &x : refs[(size_t)i]) {
            uint8_t *dst = x.type == kPngIDAT ? (uint8_t *)c->png[kBufPngGather].p + ga : nullptr;
            job.spans[k++] = Crc32Span{job.d_blob + b + x.at + 4, dst, nullptr, x.len + 4, 0xFFFFFFFFu, 4, 0, 0};
            if (dst) ga += (size_t)x.len;
        }
        b += ((size_t)file_len[i] + 255) & ~(size_t)255;
        g += ((size_t)fi[(size_t)i].idat_bytes + 255) & ~(size_t)255;
    }
    if (!crc32_run(c, &job, s)) return all_fail(ZS_STREAM_ERROR);
    const double crc_ms = job.ms;
    k = 0;
    std::vector<const void *> d_idat;
    std::vector<int64_t> d_len, d_w, d_h;
    std::vector<int> d_bits, d_il, d_who;
    std::vector<void *> d_out;
    for (size_t j = 0; j < who.size(); j++) {
        const int i = who[j];
        const uint8_t *f = (const uint8_t *)file[i];
        for (const PngChunkRef &x : refs[(size_t)i]) {
            const uint32_t got = job.crc[k++];
            if (st[(size_t)i] == ZS_OK && got != png_be32(f + x.at + 8 + x.len)) {
                snprintf(msg, sizeof msg, "CRC error in %.4s chunk at offset %lld", (const char *)f + x.at + 4, (long long)x.at);
                st[(size_t)i] = ZS_DATA_ERROR, why[(size_t)i] = msg;
            }
        }
        if (st[(size_t)i] != ZS_OK) continue;
        const PngFileInfo &p = fi[(size_t)i];
        d_who.push_back(i), d_idat.push_back(idat[j]), d_len.push_back(p.idat_bytes), d_w.push_back(p.width), d_h.push_back(p.height);
        d_bits.push_back(p.bits_per_pixel), d_il.push_back(p.interlace), d_out.push_back(expand ? (void *)((uint8_t *)c->png[kBufPngRaw].p + raw_at[(size_t)i]) : out[i]);
    }
    if (!d_who.empty()) {
        std::vector<int> dst_st(d_who.size(), ZS_STREAM_ERROR);
        const int drc = zs_png_decode_batch_device(c, (int)d_who.size(), d_idat.data(), d_len.data(), d_w.data(), d_h.data(), d_bits.data(), d_il.data(),
                                                   d_out.data(), dst_st.data(), (void *)s);
        if (drc != ZS_OK && drc != ZS_DATA_ERROR) return all_fail(drc);
        const std::string inner = c->err;
        bool first = true;
        for (size_t j = 0; j < d_who.size(); j++) {
            if (dst_st[j] == ZS_OK) continue;
            st[(size_t)d_who[j]] = dst_st[j];
            // the decode call's message names its first failing image by its place in that call: keep the reason
            std::string reason = "the IDAT stream does not decode";
            if (first) {
                const size_t colon = inner.find(": ", inner.find("image "));
                reason = inner.find("image ") != std::string::npos && colon != std::string::npos ? inner.substr(colon + 2) : inner;
                first = false;
            }
            why[(size_t)d_who[j]] = reason;
        }
    }
    double expand_ms = 0;
    if (expand) {  // KX over the files that are whole
        PngExpandJob xjob;
        for (int i : d_who) {
            if (st[(size_t)i] != ZS_OK) continue;
            const PngFileInfo &p = fi[(size_t)i];
            const PngFileColors &col = colors[(size_t)i];
            xjob.add((const uint8_t *)c->png[kBufPngRaw].p + raw_at[(size_t)i], out[i], p.width, p.height, p.bit_depth, p.color_type, format, col.plte, col.plte_entries,
                     col.trns, col.trns_len);
        }
        if (!xjob.img.empty()) {
            if (!png_expand_run(c, xjob, format, s, &no_memory)) return all_fail(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
            if (!hip_stream && hipStreamSynchronize(s) != hipSuccess) return all_fail(ZS_STREAM_ERROR);
            expand_ms = xjob.ms;
        }
    }
    if (c->profiling) c->stage_ms[kStCrc32] = crc_ms, c->stage_ms[kStPngExpand] = expand_ms;
    return verdict();
}
}  // namespace

extern "C" int zs_png_decode_files_batch(zs_ctx *c, int n, const void *const *file, const int64_t *file_len, void *const *out, const int64_t *out_cap,
                                         zs_png_info *info, int *status, void *hip_stream) {
    return png_decode_files(c, n, file, file_len, -1, out, out_cap, info, status, hip_stream);
}

extern "C" int zs_png_decode_files_rgba_batch(zs_ctx *c, int n, const void *const *file, const int64_t *file_len, int format, void *const *out,
                                              const int64_t *out_cap, zs_png_info *info, int *status, void *hip_stream) {
    if (format < 0) {
        if (c) c->err = "stream error: format is neither ZS_PNG_RGBA8 nor ZS_PNG_RGBA16";
        return ZS_STREAM_ERROR;
    }
    return png_decode_files(c, n, file, file_len, format, out, out_cap, info, status, hip_stream);
}

// ------------------------------------------------------------------ animated PNG: the walk, the compose launch (KM, zs_png.hip), files to canvases
static_assert(sizeof(zs_png_frame) == sizeof(PngFrame) && offsetof(zs_png_frame, n_chunks) == offsetof(PngFrame, n_chunks) &&
                  offsetof(zs_png_frame, blend_op) == offsetof(PngFrame, blend_op),
              "zs_png_frame mirrors PngFrame");
static_assert(sizeof(zs_png_anim) == sizeof(PngAnimInfo) && offsetof(zs_png_anim, default_is_frame) == offsetof(PngAnimInfo, default_is_frame),
              "zs_png_anim mirrors PngAnimInfo");

extern "C" int zs_png_anim_info(const void *file, int64_t len, zs_png_anim *anim, zs_png_frame *frames, int frames_cap) {
    if (!file || !anim || len < 0 || frames_cap < 0 || (frames_cap > 0 && !frames)) return ZS_STREAM_ERROR;
    char msg[192];
    PngFileInfo info;
    PngFileColors col;
    PngAnimInfo a;
    const uint8_t *f = (const uint8_t *)file;
    if (!png_walk_file(f, len, &info, msg, sizeof msg, true, [](const PngChunkRef &) {}) || !png_file_colors(f, len, info, &col, msg, sizeof msg) ||
        !png_walk_anim(f, len, info, &a, msg, sizeof msg, [&](int k, const PngFrame &fr) { if (k < frames_cap) memcpy(&frames[k], &fr, sizeof fr); },
                       [](int, const PngChunkRef &) {}))
        return ZS_DATA_ERROR;
    memcpy(anim, &a, sizeof a);
    return frames_cap < a.n_frames ? ZS_BUF_ERROR : ZS_OK;
}

namespace {
constexpr PngGrid kComposeGrid{kPngSlice, kComposeWavesPerWg, 64};

// The animations of one KM launch: descriptors, the flat list of waves (canvas rows times the waves that share a row), and
// all their frames.
struct PngComposeJob {
    std::vector<PngComposeAnim> anim;
    PngOffsets waves;
    std::vector<PngComposeFrame> frames;
    double ms = 0;  // profiling: the launches
    void add(void *out, int64_t w, int64_t h, int n_frames, int format) {
        anim.push_back(PngComposeAnim{(uint8_t *)out, (int32_t)w, (int32_t)h, (int32_t)frames.size(), (int32_t)n_frames});
        waves.add(h * png_compose_row_waves(w, format));
    }
    void add_frame(const void *px, const PngFrame &f) {
        frames.push_back(PngComposeFrame{(const uint8_t *)px, (int32_t)f.x, (int32_t)f.y, (int32_t)f.width, (int32_t)f.height, f.dispose_op, f.blend_op});
    }
};

// KM over the job on `s` (png_run_list: one wait)
bool png_compose_run(zs_ctx *c, PngComposeJob &job, int format, hipStream_t s, bool *no_memory) {
    const int m = (int)job.anim.size();
    const size_t b_anim = sizeof(PngComposeAnim) * (size_t)m, b_off = job.waves.bytes(true);
    return png_run_list(c, c->png[kBufPngCimg], {{job.anim.data(), b_anim}, {job.frames.data(), sizeof(PngComposeFrame) * job.frames.size()}}, job.waves, 0,
                        kComposeGrid, s, no_memory, &job.ms, [&](dim3 grid, dim3 block, uint8_t *d, int64_t wave0) {
                            const PngComposeAnim *d_anim = (const PngComposeAnim *)d;
                            const int32_t *d_off = (const int32_t *)(d + b_anim);
                            const PngComposeFrame *d_fr = (const PngComposeFrame *)(d + b_anim + b_off);
                            if (format == ZS_PNG_FMT_RGBA16) hipLaunchKernelGGL(zs_png_compose_kernel<ZS_PNG_FMT_RGBA16>, grid, block, 0, s, d_anim, d_off, d_fr, m, wave0);
                            else hipLaunchKernelGGL(zs_png_compose_kernel<ZS_PNG_FMT_RGBA8>, grid, block, 0, s, d_anim, d_off, d_fr, m, wave0);
                        });
}

bool png_frame_fits(const PngFrame &f, int64_t w, int64_t h) {
    return f.x >= 0 && f.y >= 0 && f.width >= 1 && f.height >= 1 && f.x <= w - f.width && f.y <= h - f.height && f.dispose_op >= 0 && f.dispose_op <= 2 &&
           f.blend_op >= 0 && f.blend_op <= 1;
}
}  // namespace

extern "C" int zs_png_compose_batch_device(zs_ctx *c, int n, const void *const *const *frame_px, const zs_png_frame *const *frames, const int *n_frames,
                                           const int64_t *width, const int64_t *height, int format, void *const *out, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!frame_px || !frames || !n_frames || !width || !height || !out) return ZS_STREAM_ERROR;
    if (!png_format_ok(c, format)) return ZS_STREAM_ERROR;
    const uintptr_t mis = (uintptr_t)(png_expand_bytes(format) - 1);
    int64_t total_rows = 0, total_frames = 0;
    for (int i = 0; i < n; i++) {
        bool ok = frame_px[i] && frames[i] && out[i] && ((uintptr_t)out[i] & mis) == 0 && n_frames[i] >= 1 && png_dims_ok(width[i], height[i]);
        for (int f = 0; ok && f < n_frames[i]; f++)
            ok = frame_px[i][f] && ((uintptr_t)frame_px[i][f] & mis) == 0 && png_frame_fits(*(const PngFrame *)&frames[i][f], width[i], height[i]);
        if (!ok) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        total_rows += height[i] * png_compose_row_waves(width[i], format), total_frames += n_frames[i];
        if (total_rows > 0x7FFFFFFF || total_frames > 0x7FFFFFFF) {  // (the grid is the list of rows, a wave per 64 groups of a row)
            c->err = "stream error: more than 2^31 - 1 canvas rows (counted once per 64 groups of 16 bytes) or frames in one call (split the batch)";
            return ZS_STREAM_ERROR;
        }
    }
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    PngComposeJob job;
    for (int i = 0; i < n; i++) {
        job.add(out[i], width[i], height[i], n_frames[i], format);
        for (int f = 0; f < n_frames[i]; f++) job.add_frame(frame_px[i][f], *(const PngFrame *)&frames[i][f]);
    }
    bool no_memory = false;
    if (!png_compose_run(c, job, format, s, &no_memory)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    png_set_stage(c, kStPngCompose, job.ms);
    return png_done(hip_stream, s);
}

// Files -> composed canvases: the three walks on the host, one upload, KC over the critical chunks and every frame's data
// chunks (IDAT, or fdAT without its sequence number: gathered per frame), the decode call over all frames of all files as
// images of their own size, KX into a buffer of the context, KM into out[i].
extern "C" int zs_png_decode_anim_batch(zs_ctx *c, int n, const void *const *file, const int64_t *file_len, int format, void *const *out,
                                        const int64_t *out_cap, zs_png_anim *anim, int *status, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!file || !file_len || !out || !out_cap) return ZS_STREAM_ERROR;
    if (!png_format_ok(c, format)) return ZS_STREAM_ERROR;
    const int px = png_expand_bytes(format);
    for (int i = 0; i < n; i++)
        if (!file[i] || !out[i] || file_len[i] < 0 || out_cap[i] < 0 || ((uintptr_t)out[i] & (uintptr_t)(px - 1)) != 0) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
    struct DataRef {
        int frame;  // -1: a critical chunk that is checked and not gathered
        PngChunkRef ref;
    };
    struct File {
        PngFileInfo info;
        PngFileColors col;
        PngAnimInfo anim;
        std::vector<PngFrame> frames;
        std::vector<DataRef> refs;
        int frame0 = 0;  // its first frame in the call's list of frames
    };
    std::vector<File> fs((size_t)n);
    std::vector<std::string> why((size_t)n);
    std::vector<int> st((size_t)n, ZS_OK);
    size_t blob = 0;
    int64_t n_spans = 0, rows = 0, canvas_rows = 0, n_fr = 0;
    char msg[256];
    for (int i = 0; i < n; i++) {
        File &F = fs[(size_t)i];
        const uint8_t *f = (const uint8_t *)file[i];
        std::vector<PngChunkRef> crit;
        memset(&F.anim, 0, sizeof F.anim);
        const bool walked = png_walk_file(f, file_len[i], &F.info, msg, sizeof msg, false, [&](const PngChunkRef &x) { crit.push_back(x); });
        F.anim.png = F.info;
        if (!walked || !png_file_colors(f, file_len[i], F.info, &F.col, msg, sizeof msg) ||
            !png_walk_anim(f, file_len[i], F.info, &F.anim, msg, sizeof msg, [&](int, const PngFrame &fr) { F.frames.push_back(fr); },
                           [&](int k, const PngChunkRef &x) { F.refs.push_back(DataRef{k, x}); })) {
            st[(size_t)i] = ZS_DATA_ERROR, why[(size_t)i] = msg;
        } else {
            for (const PngChunkRef &x : crit)
                if (x.type != kPngIDAT || !F.anim.default_is_frame) F.refs.push_back(DataRef{-1, x});
            for (size_t k = 0; k < F.frames.size() && st[(size_t)i] == ZS_OK; k++) {
                const PngFrame &fr = F.frames[k];
                if (fr.data_bytes > kCrcMaxLen || zs_png_idat_layout(fr.width, fr.height, F.info.bits_per_pixel, F.info.interlace, nullptr, nullptr) > kCrcMaxLen) {
                    snprintf(msg, sizeof msg, "frame %d: the frame or its data is above 2 GiB - 1 KiB", (int)k);
                    st[(size_t)i] = ZS_DATA_ERROR, why[(size_t)i] = msg;
                }
            }
            const bool too_big = F.info.width > (kCrcMaxLen / px) / F.info.height;  // (a canvas can be larger than every frame: the default image need not be one)
            const int64_t canvas = too_big ? 0 : F.info.width * F.info.height * px;
            if (st[(size_t)i] == ZS_OK && (too_big || canvas > INT64_MAX / F.anim.n_frames)) {
                st[(size_t)i] = ZS_DATA_ERROR, why[(size_t)i] = "the canvases are above what a call can address";
            } else if (st[(size_t)i] == ZS_OK && out_cap[i] < canvas * F.anim.n_frames) {
                snprintf(msg, sizeof msg, "the %d canvases need %lld bytes, out_cap is %lld", F.anim.n_frames, (long long)(canvas * F.anim.n_frames), (long long)out_cap[i]);
                st[(size_t)i] = ZS_BUF_ERROR, why[(size_t)i] = msg;
            }
        }
        if (anim) memcpy(&anim[i], &F.anim, sizeof F.anim);
        if (st[(size_t)i] != ZS_OK) continue;
        for (const PngFrame &fr : F.frames) {
            int64_t r7[kAdam7Passes];
            (void)zs_png_idat_layout(fr.width, fr.height, F.info.bits_per_pixel, F.info.interlace, nullptr, r7);
            for (int64_t v : r7) rows += v;
        }
        F.frame0 = (int)n_fr;
        n_fr += (int64_t)F.frames.size();
        canvas_rows += F.info.height * png_compose_row_waves(F.info.width, format);
        blob += ((size_t)file_len[i] + 255) & ~(size_t)255;
        n_spans += (int64_t)F.refs.size();
    }
    auto finish = [&](int rc) {
        if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
        return rc;
    };
    auto verdict = [&]() {  // the first failing file's code and message
        for (int i = 0; i < n; i++)
            if (st[(size_t)i] != ZS_OK) {
                c->err = std::string(st[(size_t)i] == ZS_BUF_ERROR ? "buffer error: file " : "data error: file ") + std::to_string(i) + ": " + why[(size_t)i];
                return finish(st[(size_t)i]);
            }
        return finish(ZS_OK);
    };
    if (n_spans > 0x3FFFFFFF || rows > 0x7FFFFFFF || canvas_rows > 0x7FFFFFFF || n_fr > 0x3FFFFFFF) {
        c->err = "stream error: too many chunks, frames or rows in one call (split the batch)";
        return ZS_STREAM_ERROR;
    }
    if (n_spans == 0) return verdict();
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    auto all_fail = [&](int code) {
        for (int &v : st)
            if (v == ZS_OK) v = code;
        return finish(code);
    };
    // where every frame of the call has its gathered stream, its raw scanlines and its RGBA pixels (each on a 256-byte boundary)
    std::vector<size_t> g_at((size_t)n_fr), raw_at((size_t)n_fr), px_at((size_t)n_fr);
    size_t gather = 0, raw_total = 0, px_total = 0;
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        const File &F = fs[(size_t)i];
        for (size_t k = 0; k < F.frames.size(); k++) {
            const PngFrame &fr = F.frames[k];
            const size_t j = (size_t)F.frame0 + k;
            g_at[j] = gather, gather += ((size_t)fr.data_bytes + 255) & ~(size_t)255;
            raw_at[j] = raw_total, raw_total += ((size_t)(png_bits_row_bytes(fr.width, F.info.bits_per_pixel) * fr.height) + 255) & ~(size_t)255;
            px_at[j] = px_total, px_total += ((size_t)(fr.width * fr.height * px) + 255) & ~(size_t)255;
        }
    }
    Crc32Job job;
    bool no_memory = false;
    if (!ensure(c, c->png[kBufPngGather], gather + 256) || !ensure(c, c->png[kBufPngRaw], raw_total + 256) || !ensure(c, c->png[kBufPngFrames], px_total + 256)) return all_fail(ZS_MEM_ERROR);
    if (!crc32_begin(c, (int)n_spans, blob, &job, &no_memory)) return all_fail(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    size_t k = 0, b = 0;
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        const File &F = fs[(size_t)i];
        memcpy(job.blob + b, file[i], (size_t)file_len[i]);
        std::vector<size_t> fill(F.frames.size(), 0);  // bytes of every frame gathered so far
        for (const DataRef &r : F.refs) {
            const PngChunkRef &x = r.ref;
            const uint32_t skip = x.type == kPngfdAT ? 8 : 4;  // the type, and an fdAT's sequence number
            uint8_t *dst = nullptr;
            if (r.frame >= 0) {
                dst = (uint8_t *)c->png[kBufPngGather].p + g_at[(size_t)F.frame0 + (size_t)r.frame] + fill[(size_t)r.frame];
                fill[(size_t)r.frame] += (size_t)(x.len + 4 - skip);
            }
            job.spans[k++] = Crc32Span{job.d_blob + b + x.at + 4, dst, nullptr, x.len + 4, 0xFFFFFFFFu, skip, 0, 0};
        }
        b += ((size_t)file_len[i] + 255) & ~(size_t)255;
    }
    if (!crc32_run(c, &job, s)) return all_fail(ZS_STREAM_ERROR);
    const double crc_ms = job.ms;
    k = 0;
    struct Img {
        int file, frame;
    };
    std::vector<Img> d_who;
    std::vector<const void *> d_idat;
    std::vector<int64_t> d_len, d_w, d_h;
    std::vector<int> d_bits, d_il;
    std::vector<void *> d_out;
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        const File &F = fs[(size_t)i];
        const uint8_t *f = (const uint8_t *)file[i];
        for (const DataRef &r : F.refs) {
            const PngChunkRef &x = r.ref;
            const uint32_t got = job.crc[k++];
            if (st[(size_t)i] == ZS_OK && got != png_be32(f + x.at + 8 + x.len)) {
                if (r.frame >= 0) snprintf(msg, sizeof msg, "frame %d: CRC error in %.4s chunk at offset %lld", r.frame, (const char *)f + x.at + 4, (long long)x.at);
                else snprintf(msg, sizeof msg, "CRC error in %.4s chunk at offset %lld", (const char *)f + x.at + 4, (long long)x.at);
                st[(size_t)i] = ZS_DATA_ERROR, why[(size_t)i] = msg;
            }
        }
        if (st[(size_t)i] != ZS_OK) continue;
        for (size_t q = 0; q < F.frames.size(); q++) {
            const PngFrame &fr = F.frames[q];
            const size_t j = (size_t)F.frame0 + q;
            d_who.push_back(Img{i, (int)q}), d_idat.push_back((const uint8_t *)c->png[kBufPngGather].p + g_at[j]), d_len.push_back(fr.data_bytes);
            d_w.push_back(fr.width), d_h.push_back(fr.height), d_bits.push_back(F.info.bits_per_pixel), d_il.push_back(F.info.interlace);
            d_out.push_back((uint8_t *)c->png[kBufPngRaw].p + raw_at[j]);
        }
    }
    if (!d_who.empty()) {
        std::vector<int> dst_st(d_who.size(), ZS_STREAM_ERROR);
        const int drc = zs_png_decode_batch_device(c, (int)d_who.size(), d_idat.data(), d_len.data(), d_w.data(), d_h.data(), d_bits.data(), d_il.data(),
                                                   d_out.data(), dst_st.data(), (void *)s);
        if (drc != ZS_OK && drc != ZS_DATA_ERROR) return all_fail(drc);
        const std::string inner = c->err;
        bool first = true;
        for (size_t j = 0; j < d_who.size(); j++) {
            if (dst_st[j] == ZS_OK) continue;
            // the decode call's message names its first failing image by its place in that call: keep the reason
            std::string reason = "the frame's stream does not decode";
            if (first) {
                const size_t colon = inner.find(": ", inner.find("image "));
                reason = inner.find("image ") != std::string::npos && colon != std::string::npos ? inner.substr(colon + 2) : inner;
                first = false;
            }
            if (st[(size_t)d_who[j].file] != ZS_OK) continue;  // (the file's first failing frame stays)
            st[(size_t)d_who[j].file] = dst_st[j];
            why[(size_t)d_who[j].file] = "frame " + std::to_string(d_who[j].frame) + ": " + reason;
        }
    }
    double expand_ms = 0, compose_ms = 0;
    PngExpandJob xjob;
    PngComposeJob mjob;
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        const File &F = fs[(size_t)i];
        mjob.add(out[i], F.info.width, F.info.height, (int)F.frames.size(), format);
        for (size_t q = 0; q < F.frames.size(); q++) {
            const PngFrame &fr = F.frames[q];
            const size_t j = (size_t)F.frame0 + q;
            uint8_t *pixels = (uint8_t *)c->png[kBufPngFrames].p + px_at[j];
            xjob.add((const uint8_t *)c->png[kBufPngRaw].p + raw_at[j], pixels, fr.width, fr.height, F.info.bit_depth, F.info.color_type, format, F.col.plte,
                     F.col.plte_entries, F.col.trns, F.col.trns_len);
            mjob.add_frame(pixels, fr);
        }
    }
    if (!mjob.anim.empty()) {
        if (!png_expand_run(c, xjob, format, s, &no_memory) || !png_compose_run(c, mjob, format, s, &no_memory))
            return all_fail(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
        if (!hip_stream && hipStreamSynchronize(s) != hipSuccess) return all_fail(ZS_STREAM_ERROR);
        expand_ms = xjob.ms, compose_ms = mjob.ms;
    }
    if (c->profiling) c->stage_ms[kStCrc32] = crc_ms, c->stage_ms[kStPngExpand] = expand_ms, c->stage_ms[kStPngCompose] = compose_ms;
    return verdict();
}

// ------------------------------------------------------------------ animated PNG on the way out: the frame diff (KD), the crop, the encoder
namespace {
constexpr PngGrid kDiffGrid{kPngSlice, kDiffWavesPerWg, 64}, kCropGrid{kPngSlice, kCropRowsPerWg, 64};

struct PngRegion {
    int64_t x, y, w, h;
};

// What zs_png_diff_batch_device and the encoder check alike: the canvases of n animations.  *waves: KD's grid.
bool png_canvases_ok(zs_ctx *c, int n, const void *const *canvases, const int *n_frames, const int64_t *width, const int64_t *height, int format, int64_t *waves) {
    if (!canvases || !n_frames || !width || !height) return false;
    if (!png_format_ok(c, format)) return false;
    const uintptr_t mis = (uintptr_t)(png_expand_bytes(format) - 1);
    int64_t total_waves = 0, total_frames = 0;
    for (int i = 0; i < n; i++) {
        if (!canvases[i] || ((uintptr_t)canvases[i] & mis) != 0 || n_frames[i] < 1 || !png_dims_ok(width[i], height[i])) {
            c->err = "stream error";
            return false;
        }
        total_waves += height[i] * png_compose_row_waves(width[i], format), total_frames += n_frames[i];
        if (total_waves > 0x7FFFFFFF || total_frames > 0x7FFFFFFF) {  // (the grid is the list of rows, a wave per 64 groups of a row)
            c->err = "stream error: more than 2^31 - 1 canvas rows (counted once per 64 groups of 16 bytes) or frames in one call (split the batch)";
            return false;
        }
    }
    *waves = total_waves;
    return true;
}

// KD over the canvases of n animations: regions[i][f] for every frame.  Uploads the descriptors through the staging buffer,
// runs both launches on `s` and waits for `s` twice: for the upload and the launches, and for the rectangles.  Animations of
// one frame take no part; a call without any other launches nothing and does not wait.
bool png_diff_run(zs_ctx *c, int n, const void *const *canvases, const int *n_frames, const int64_t *width, const int64_t *height, int format,
                  std::vector<std::vector<PngRegion>> &regions, hipStream_t s, bool *no_memory, double *ms) {
    *no_memory = false, *ms = 0;
    regions.assign((size_t)n, {});
    std::vector<PngDiffAnim> anims((size_t)n);
    std::vector<int32_t> wave_off((size_t)n + 1), pair_off((size_t)n + 1);
    int64_t waves = 0, pairs = 0, recs = 0;
    for (int i = 0; i < n; i++) {
        regions[(size_t)i].assign((size_t)n_frames[i], PngRegion{0, 0, width[i], height[i]});
        const int64_t w_i = n_frames[i] > 1 ? height[i] * png_compose_row_waves(width[i], format) : 0;
        anims[(size_t)i] = PngDiffAnim{(const uint8_t *)canvases[i], recs, (int32_t)width[i], (int32_t)height[i], n_frames[i], 0};
        wave_off[(size_t)i] = (int32_t)waves, pair_off[(size_t)i] = (int32_t)pairs;
        waves += w_i, pairs += n_frames[i] - 1, recs += w_i * (n_frames[i] - 1);
    }
    wave_off[(size_t)n] = (int32_t)waves, pair_off[(size_t)n] = (int32_t)pairs;
    if (pairs == 0) return true;
    const size_t b_anim = sizeof(PngDiffAnim) * (size_t)n, b_off = (sizeof(int32_t) * ((size_t)n + 1) + 15) & ~(size_t)15, b_up = b_anim + 2 * b_off,
                 b_rec = sizeof(PngDiffRec) * (size_t)recs, b_rect = sizeof(PngDiffRect) * (size_t)pairs;
    if (!ensure(c, c->png[kBufPngDimg], b_up) || !ensure(c, c->png[kBufPngDrec], b_rec + b_rect) || !ensure_pinned(c, std::max(b_up, b_rect))) {
        *no_memory = true;
        return false;
    }
    uint8_t *hp = (uint8_t *)c->pinned;
    memcpy(hp, anims.data(), b_anim);
    memcpy(hp + b_anim, wave_off.data(), sizeof(int32_t) * ((size_t)n + 1));
    memcpy(hp + b_anim + b_off, pair_off.data(), sizeof(int32_t) * ((size_t)n + 1));
    ZS_HIP(c, hipMemcpyAsync(c->png[kBufPngDimg].p, c->pinned, b_up, hipMemcpyHostToDevice, s));
    const bool prof = c->profiling;
    if (prof) (void)hipEventRecord(c->ev_png[0], s);
    const PngDiffAnim *d_anim = (const PngDiffAnim *)c->png[kBufPngDimg].p;
    const int32_t *d_woff = (const int32_t *)((const uint8_t *)c->png[kBufPngDimg].p + b_anim), *d_poff = (const int32_t *)((const uint8_t *)c->png[kBufPngDimg].p + b_anim + b_off);
    PngDiffRec *d_rec = (PngDiffRec *)c->png[kBufPngDrec].p;
    PngDiffRect *d_rect = (PngDiffRect *)((uint8_t *)c->png[kBufPngDrec].p + b_rec);  // (8-aligned: a record is 8 bytes)
    if (!png_launch_list(c, waves, kDiffGrid, [&](dim3 grid, dim3 block, int64_t wave0) {
            if (format == ZS_PNG_FMT_RGBA16) hipLaunchKernelGGL(zs_png_diff_kernel<ZS_PNG_FMT_RGBA16>, grid, block, 0, s, d_anim, d_woff, n, wave0, d_rec);
            else hipLaunchKernelGGL(zs_png_diff_kernel<ZS_PNG_FMT_RGBA8>, grid, block, 0, s, d_anim, d_woff, n, wave0, d_rec);
        }))
        return false;
    hipLaunchKernelGGL(zs_png_diff_merge_kernel, dim3((unsigned)pairs), dim3(256), 0, s, d_anim, d_poff, n, format, (const PngDiffRec *)d_rec, d_rect);
    ZS_HIP(c, hipGetLastError());
    if (prof) (void)hipEventRecord(c->ev_png[1], s);
    ZS_HIP(c, hipStreamSynchronize(s));  // the upload has left the staging buffer
    ZS_HIP(c, hipMemcpyAsync(c->pinned, d_rect, b_rect, hipMemcpyDeviceToHost, s));
    ZS_HIP(c, hipStreamSynchronize(s));
    if (prof) {
        float t = 0;
        (void)hipEventElapsedTime(&t, c->ev_png[0], c->ev_png[1]);
        *ms = t;
    }
    const PngDiffRect *rects = (const PngDiffRect *)c->pinned;
    for (int i = 0; i < n; i++)
        for (int f = 1; f < n_frames[i]; f++) {
            PngRegion &r = regions[(size_t)i][(size_t)f];
            png_diff_finish(rects[(size_t)pair_off[(size_t)i] + (size_t)f - 1], &r.x, &r.y, &r.w, &r.h);
        }
    return true;
}

// The images of one crop launch: descriptors and the flat row list.
struct PngCropJob {
    std::vector<PngCropImg> img;
    PngOffsets rows;
    double ms = 0;  // profiling: the launches
    void add(const void *in, int64_t in_width, int64_t x, int64_t y, int64_t w, int64_t h, int px, void *out) {
        img.push_back(PngCropImg{(const uint8_t *)in + (y * in_width + x) * px, (uint8_t *)out, in_width * px, (int32_t)w, (int32_t)h});
        rows.add(h);
    }
};

// The crop over the job on `s` (png_run_list: one wait)
bool png_crop_run(zs_ctx *c, PngCropJob &job, int px, hipStream_t s, bool *no_memory) {
    const int m = (int)job.img.size();
    const size_t b_img = sizeof(PngCropImg) * (size_t)m;
    return png_run_list(c, c->png[kBufPngKimg], {{job.img.data(), b_img}}, job.rows, 0, kCropGrid, s, no_memory, &job.ms,
                        [&](dim3 grid, dim3 block, uint8_t *d, int64_t row0) {
                            const PngCropImg *d_img = (const PngCropImg *)d;
                            const int32_t *d_off = (const int32_t *)(d + b_img);
                            if (px == 8) hipLaunchKernelGGL(zs_png_crop_kernel<8>, grid, block, 0, s, d_img, d_off, m, row0);
                            else hipLaunchKernelGGL(zs_png_crop_kernel<4>, grid, block, 0, s, d_img, d_off, m, row0);
                        });
}

// chunks that hold a frame's stream of z bytes: IDAT, or fdAT, whose four bytes of sequence number count against the chunk
// limit; *step: stream bytes of every chunk but the last.  -1: one chunk was asked for and cannot hold the stream.
int64_t png_anim_chunks(int64_t z, int64_t idat_chunk_bytes, bool fdat, int64_t *step) {
    const int64_t most = kPngMaxChunk - (fdat ? 4 : 0);
    if (idat_chunk_bytes == 0 && z > most) return -1;
    *step = idat_chunk_bytes == 0 ? z : std::min(idat_chunk_bytes, most);
    return z == 0 || idat_chunk_bytes == 0 ? 1 : (z + *step - 1) / *step;
}
constexpr int64_t kPngActlBytes = 20, kPngFctlBytes = 38;
}  // namespace

extern "C" int zs_png_diff_batch_device(zs_ctx *c, int n, const void *const *canvases, const int *n_frames, const int64_t *width, const int64_t *height,
                                        int format, zs_png_frame *const *frames_out, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    int64_t waves = 0;
    if (!frames_out || !png_canvases_ok(c, n, canvases, n_frames, width, height, format, &waves)) return ZS_STREAM_ERROR;
    for (int i = 0; i < n; i++)
        if (!frames_out[i]) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    std::vector<std::vector<PngRegion>> regions;
    bool no_memory = false;
    double ms = 0;
    if (!png_diff_run(c, n, canvases, n_frames, width, height, format, regions, s, &no_memory, &ms)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    png_set_stage(c, kStPngDiff, ms);
    for (int i = 0; i < n; i++)
        for (int f = 0; f < n_frames[i]; f++) {
            const PngRegion &r = regions[(size_t)i][(size_t)f];
            zs_png_frame &o = frames_out[i][f];
            o.x = r.x, o.y = r.y, o.width = r.w, o.height = r.h, o.dispose_op = kPngDisposeNone, o.blend_op = kPngBlendSource;
        }
    return ZS_OK;
}

extern "C" int zs_png_crop_batch_device(zs_ctx *c, int n, const void *const *in, const int64_t *in_width, const int64_t *x, const int64_t *y, const int64_t *width,
                                        const int64_t *height, int pixel_bytes, void *const *out, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!in || !in_width || !x || !y || !width || !height || !out) return ZS_STREAM_ERROR;
    if (pixel_bytes != 4 && pixel_bytes != 8) {
        c->err = "stream error: pixel_bytes is neither 4 nor 8";
        return ZS_STREAM_ERROR;
    }
    const uintptr_t mis = (uintptr_t)(pixel_bytes - 1);
    int64_t total_rows = 0;
    for (int i = 0; i < n; i++) {
        const bool ok = in[i] && out[i] && ((uintptr_t)in[i] & mis) == 0 && ((uintptr_t)out[i] & mis) == 0 && in_width[i] >= 1 && in_width[i] <= 0x7FFFFFFF && width[i] >= 1 &&
                        height[i] >= 1 && height[i] <= 0x7FFFFFFF && x[i] >= 0 && y[i] >= 0 && y[i] <= 0x7FFFFFFF - height[i] && x[i] <= in_width[i] - width[i];
        if (!ok) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        total_rows += height[i];
    }
    if (!png_rows_ok(c, total_rows)) return ZS_STREAM_ERROR;  // (the grid is the row list)
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    PngCropJob job;
    for (int i = 0; i < n; i++) job.add(in[i], in_width[i], x[i], y[i], width[i], height[i], pixel_bytes, out[i]);
    bool no_memory = false;
    if (!png_crop_run(c, job, pixel_bytes, s, &no_memory)) return no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
    png_set_stage(c, kStPngCrop, job.ms);
    return png_done(hip_stream, s);
}

extern "C" int64_t zs_png_anim_bound(int64_t width, int64_t height, int n_frames, int format, int interlace, int64_t idat_chunk_bytes, int64_t extra_len) {
    if (!png_dims_ok(width, height) || n_frames < 1 || (format != ZS_PNG_FMT_RGBA8 && format != ZS_PNG_FMT_RGBA16) ||
        (interlace != 0 && interlace != 1) || idat_chunk_bytes < 0 || idat_chunk_bytes > kPngMaxChunk || extra_len < 0 || extra_len > (int64_t)1 << 60)
        return -1;
    const int px = png_expand_bytes(format);
    if (width * height > kCrcMaxLen / px) return -1;  // (what the encoder refuses: a filtered canvas above 2 GiB - 1 KiB)
    const int64_t filtered = zs_png_idat_layout(width, height, 8 * px, interlace, nullptr, nullptr);
    if (filtered > kCrcMaxLen) return -1;
    const int64_t z = zs_deflate_bound(filtered);
    int64_t step = 0;
    const int64_t idats = png_anim_chunks(z, idat_chunk_bytes, false, &step), fdats = n_frames > 1 ? png_anim_chunks(z, idat_chunk_bytes, true, &step) : 0;
    if (idats < 0 || fdats < 0) return -1;
    return 8 + 25 + extra_len + 1048 + kPngActlBytes + kPngFctlBytes + z + 12 * idats + (int64_t)(n_frames - 1) * (kPngFctlBytes + z + 16 * fdats) + 12;
}

// Canvases -> animated files: the survey (KV) over an animation's canvases as one tall image, the choice and PLTE / tRNS per
// animation, the diff (KD), the crop of every later frame's region into a buffer of the context (a region as wide as the
// canvas is read in place: its rows lie back to back already), the pack (KG) and the IDAT call over all frames of all
// animations as images of their regions' sizes, then one KC launch that frames every IDAT and fdAT chunk and places the host's
// bytes -- signature, IHDR, the caller's chunks, PLTE, tRNS, acTL, every fcTL, IEND -- around them.
extern "C" int zs_png_encode_anim_batch_device(zs_ctx *c, int n, const void *const *canvases, const int *n_frames, const int64_t *width, const int64_t *height,
                                               int format, const int *const *delay_num, const int *const *delay_den, const int *n_plays, const int *filter,
                                               const int *interlace, const void *const *extra, const int64_t *extra_len, int64_t rows_per_write,
                                               int64_t idat_chunk_bytes, void *const *out, const int64_t *out_cap, int64_t *out_len, int *status,
                                               zs_png_frame *const *frames_out, int *color_type_out, int *bit_depth_out, int level, int strategy, int hash_variant,
                                               void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!delay_num || !delay_den || !n_plays || !filter || !out || !out_cap || !out_len || (extra && !extra_len)) return ZS_STREAM_ERROR;
    int64_t waves = 0;
    if (!png_canvases_ok(c, n, canvases, n_frames, width, height, format, &waves)) return ZS_STREAM_ERROR;
    if (rows_per_write < 0 || idat_chunk_bytes < 0 || idat_chunk_bytes > kPngMaxChunk || level < -1 || level > 9 || strategy < 0 || strategy > 4) {
        c->err = "stream error";
        return ZS_STREAM_ERROR;
    }
    const int px = png_expand_bytes(format);
    int64_t total_rows = 0, total_frames = 0;
    std::vector<int> fr0((size_t)n);  // an animation's first frame in the call's list of frames
    for (int i = 0; i < n; i++) {
        const int il = interlace ? interlace[i] : 0;
        if (il != 0 && il != 1) {
            c->err = "stream error: interlace is neither 0 nor 1";
            return ZS_STREAM_ERROR;
        }
        if (!out[i] || !delay_num[i] || !delay_den[i] || (frames_out && !frames_out[i]) || filter[i] < 0 || filter[i] > 5 || out_cap[i] < 0 || n_plays[i] < 0) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        for (int f = 0; f < n_frames[i]; f++)
            if (delay_num[i][f] < 0 || delay_num[i][f] > 65535 || delay_den[i][f] < 0 || delay_den[i][f] > 65535) {
                c->err = "stream error: a delay is outside 0 .. 65535";
                return ZS_STREAM_ERROR;
            }
        if ((int64_t)n_frames[i] * height[i] > 0x7FFFFFFF) {  // (the survey takes the canvases as one image)
            c->err = "stream error: an animation's canvases have more than 2^31 - 1 rows";
            return ZS_STREAM_ERROR;
        }
        // (no pair is chosen and no region known yet: the limit is held against a whole canvas as it comes, which no frame exceeds)
        if (width[i] * height[i] > kCrcMaxLen / px || zs_png_idat_layout(width[i], height[i], 8 * px, il, nullptr, nullptr) > kCrcMaxLen) {
            c->err = "stream error: a filtered image is above 2 GiB - 1 KiB";
            return ZS_STREAM_ERROR;
        }
        if (extra && (extra_len[i] < 0 || (extra_len[i] > 0 && !extra[i]) || !png_chunks_well_formed((const uint8_t *)extra[i], extra_len[i]))) {
            c->err = "stream error: the extra chunks of an image are not a sequence of whole chunks";
            return ZS_STREAM_ERROR;
        }
        fr0[(size_t)i] = (int)total_frames;
        total_rows += (int64_t)n_frames[i] * (il ? adam7_pass_rows(width[i], height[i]) : height[i]), total_frames += n_frames[i];
        if (total_rows > 0x7FFFFFFF || total_frames > 0x3FFFFFFF) {
            c->err = "stream error: more than 2^31 - 1 rows or 2^30 - 1 frames in one call (split the batch)";
            return ZS_STREAM_ERROR;
        }
    }
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    auto all_fail = [&](int rc) {
        for (int i = 0; i < n; i++) {
            out_len[i] = 0;
            if (status) status[i] = rc;
        }
        return rc;
    };
    const size_t M = (size_t)total_frames;
    // ---- the survey over every animation's canvases as one image, and the choice
    std::vector<zs_png_survey> sv((size_t)n);
    std::vector<int64_t> tall((size_t)n);
    for (int i = 0; i < n; i++) tall[(size_t)i] = (int64_t)n_frames[i] * height[i];
    int rc = zs_png_survey_batch_device(c, n, canvases, width, tall.data(), format, sv.data(), (void *)s);
    if (rc != ZS_OK) return all_fail(rc);
    const double survey_ms = c->profiling ? c->stage_ms[kStPngSurvey] : 0;
    std::vector<PngChosen> ch((size_t)n);
    bool any_palette = false;
    for (int i = 0; i < n; i++) {
        if (!png_choose_chunks(sv[(size_t)i], extra ? extra[i] : nullptr, extra ? extra_len[i] : 0, &ch[(size_t)i])) return all_fail(ZS_STREAM_ERROR);  // (unreachable: the survey is our own)
        if (color_type_out) color_type_out[i] = ch[(size_t)i].ct;
        if (bit_depth_out) bit_depth_out[i] = ch[(size_t)i].bd;
        any_palette = any_palette || ch[(size_t)i].ct == 3;
    }
    // ---- the diff
    std::vector<std::vector<PngRegion>> regions;
    bool no_memory = false;
    double diff_ms = 0;
    if (!png_diff_run(c, n, canvases, n_frames, width, height, format, regions, s, &no_memory, &diff_ms)) return all_fail(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    // ---- where every frame's pixels are: frame 0 and the regions as wide as the canvas in place, the others cropped
    std::vector<const void *> f_px(M), f_packed(M);
    std::vector<void *> f_zs(M);
    std::vector<int64_t> f_w(M), f_h(M), f_zcap(M), f_zlen(M, 0), f_unmatched(M, 0);
    std::vector<int> f_bits(M), f_il(M), f_filter(M), f_st(M, ZS_STREAM_ERROR);
    size_t crop_total = 0, pack_total = 0, z_total = 0;
    auto round256 = [](int64_t v) { return ((size_t)v + 255) & ~(size_t)255; };
    for (int i = 0; i < n; i++)
        for (int f = 0; f < n_frames[i]; f++) {
            const size_t j = (size_t)fr0[(size_t)i] + (size_t)f;
            const PngRegion &r = regions[(size_t)i][(size_t)f];
            const int bits = ch[(size_t)i].bd * png_channels(ch[(size_t)i].ct), il = interlace ? interlace[i] : 0;
            f_w[j] = r.w, f_h[j] = r.h, f_bits[j] = bits, f_il[j] = il, f_filter[j] = filter[i];
            f_zcap[j] = zs_deflate_bound(zs_png_idat_layout(r.w, r.h, bits, il, nullptr, nullptr));
            if (r.w != width[i]) crop_total += round256(r.w * r.h * px);
            pack_total += round256(png_bits_row_bytes(r.w, bits) * r.h), z_total += round256(f_zcap[j]);
        }
    if (!ensure(c, c->png[kBufPngCrop], crop_total + 256) || !ensure(c, c->png[kBufPngPacked], pack_total + 256) || !ensure(c, c->png[kBufPngZs], z_total + 256)) return all_fail(ZS_MEM_ERROR);
    PngCropJob kjob;
    PngPackJob gjob;
    {
        size_t k_at = 0, g_at = 0, z_at = 0;
        for (int i = 0; i < n; i++) {
            const PngChosen &h = ch[(size_t)i];
            const int64_t rb = width[i] * px, canvas = rb * height[i];
            int32_t table = -1;
            for (int f = 0; f < n_frames[i]; f++) {
                const size_t j = (size_t)fr0[(size_t)i] + (size_t)f;
                const PngRegion &r = regions[(size_t)i][(size_t)f];
                const uint8_t *cv = (const uint8_t *)canvases[i] + (int64_t)f * canvas;
                if (r.w == width[i]) f_px[j] = cv + r.y * rb;
                else {
                    uint8_t *to = (uint8_t *)c->png[kBufPngCrop].p + k_at;
                    kjob.add(cv, width[i], r.x, r.y, r.w, r.h, px, to);
                    f_px[j] = to, k_at += round256(r.w * r.h * px);
                }
                f_packed[j] = (uint8_t *)c->png[kBufPngPacked].p + g_at, g_at += round256(png_bits_row_bytes(r.w, f_bits[j]) * r.h);
                f_zs[j] = (uint8_t *)c->png[kBufPngZs].p + z_at, z_at += round256(f_zcap[j]);
                gjob.add(f_px[j], (void *)f_packed[j], r.w, r.h, h.bd, h.ct, format, h.plte.data(), h.entries, h.tlen > 0 ? h.trns.data() : nullptr, h.tlen, table);
                if (h.ct == 3) table = gjob.img.back().pal_off;  // (the animation's frames share its table)
            }
        }
    }
    if (!kjob.img.empty() && !png_crop_run(c, kjob, px, s, &no_memory)) return all_fail(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    if (!png_pack_run(c, gjob, format, any_palette ? f_unmatched.data() : nullptr, s, &no_memory)) return all_fail(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    // ---- every frame's stream
    const int zrc = zs_png_idat_interlace_batch_device(c, (int)M, f_packed.data(), f_w.data(), f_h.data(), f_bits.data(), f_il.data(), f_filter.data(), rows_per_write,
                                                       f_zs.data(), f_zcap.data(), f_zlen.data(), f_st.data(), level, strategy, hash_variant, (void *)s);
    auto stages = [&]() {
        if (c->profiling) c->stage_ms[kStPngSurvey] = survey_ms, c->stage_ms[kStPngDiff] = diff_ms, c->stage_ms[kStPngCrop] = kjob.ms, c->stage_ms[kStPngPack] = gjob.ms;
    };
    std::vector<int> st((size_t)n, ZS_OK);
    rc = zrc;  // (its message stands)
    auto fail_anim = [&](int i, int code, const std::string &why) {
        if (st[(size_t)i] == ZS_OK) st[(size_t)i] = code, out_len[i] = 0;
        if (rc == ZS_OK) rc = code, c->err = why;
    };
    auto finish = [&]() {
        if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
        stages();
        return rc;
    };
    // ---- the layout: which animations fit, and their spans
    int64_t n_spans = 0;
    for (int i = 0; i < n; i++) {
        out_len[i] = 0;
        int64_t need = 8 + 25 + (int64_t)ch[(size_t)i].xs.size() + (n_frames[i] > 1 ? kPngActlBytes + kPngFctlBytes : 0) + 12, spans = 2;
        for (int f = 0; f < n_frames[i]; f++) {
            const size_t j = (size_t)fr0[(size_t)i] + (size_t)f;
            if (f_unmatched[j] != 0)
                fail_anim(i, ZS_STREAM_ERROR, "stream error: animation " + std::to_string(i) + ": internal error: " + std::to_string(f_unmatched[j]) + " pixels of frame " +
                                                  std::to_string(f) + " have no entry in the palette made from the animation's own colours");
            else if (f_st[j] != ZS_OK) fail_anim(i, f_st[j], "stream error: animation " + std::to_string(i) + ": frame " + std::to_string(f) + ": the deflate failed");
            int64_t step = 0;
            const int64_t chunks = png_anim_chunks(f_zlen[j], idat_chunk_bytes, f > 0, &step);
            if (chunks < 0) {  // (one chunk cannot hold the stream: unreachable below 2 GiB)
                fail_anim(i, ZS_STREAM_ERROR, "stream error");
                break;
            }
            need += f_zlen[j] + (f > 0 ? kPngFctlBytes + 16 * chunks : 12 * chunks), spans += chunks + (f > 0 ? 1 : 0);
            if (frames_out) {
                const PngRegion &r = regions[(size_t)i][(size_t)f];
                zs_png_frame &o = frames_out[i][f];
                o.x = r.x, o.y = r.y, o.width = r.w, o.height = r.h, o.delay_num = delay_num[i][f], o.delay_den = delay_den[i][f];
                o.dispose_op = kPngDisposeNone, o.blend_op = kPngBlendSource, o.data_bytes = f_zlen[j], o.n_chunks = chunks;
            }
        }
        if (st[(size_t)i] != ZS_OK) continue;
        out_len[i] = need;
        if (out_cap[i] < need) {
            st[(size_t)i] = ZS_BUF_ERROR;
            if (rc == ZS_OK) rc = ZS_BUF_ERROR, c->err = "buffer error";
            continue;
        }
        n_spans += spans;
    }
    if (n_spans > 0x3FFFFFFF) {
        c->err = "stream error: too many IDAT and fdAT chunks in one call";
        for (int &v : st)
            if (v == ZS_OK) v = ZS_STREAM_ERROR;
        rc = ZS_STREAM_ERROR;
        return finish();
    }
    if (n_spans == 0) return finish();
    size_t x_total = 0;  // the host's bytes of the files: everything but the streams
    for (int i = 0; i < n; i++)
        if (st[(size_t)i] == ZS_OK) x_total += 8 + 25 + ch[(size_t)i].xs.size() + (size_t)kPngActlBytes + (size_t)kPngFctlBytes * (size_t)n_frames[i] + 12;
    Crc32Job job;
    if (!crc32_begin(c, (int)n_spans, x_total, &job, &no_memory)) {
        for (int &v : st)
            if (v == ZS_OK) v = no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
        rc = no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
        return finish();
    }
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    static const uint8_t idat_type[4] = {'I', 'D', 'A', 'T'};
    const uint32_t idat_init = ~crc32_bytes_slow(0, idat_type, 4);
    auto put_chunk = [](uint8_t *to, const char *type, const uint8_t *data, uint32_t len) {  // -> the chunk's bytes
        png_put_be32(to, len);
        memcpy(to + 4, type, 4);
        memcpy(to + 8, data, len);
        png_put_be32(to + 8 + len, crc32_bytes_slow(0, to + 4, 4 + (uint64_t)len));
        return (int64_t)len + 12;
    };
    size_t k = 0, b = 0;
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        uint8_t *o = (uint8_t *)out[i];
        const std::vector<uint8_t> &xs = ch[(size_t)i].xs;
        uint32_t seq = 0;
        auto put_fctl = [&](uint8_t *to, int f) {
            const PngRegion &r = regions[(size_t)i][(size_t)f];
            uint8_t d[26];
            png_put_be32(d, seq++), png_put_be32(d + 4, (uint32_t)r.w), png_put_be32(d + 8, (uint32_t)r.h), png_put_be32(d + 12, (uint32_t)r.x), png_put_be32(d + 16, (uint32_t)r.y);
            d[20] = (uint8_t)(delay_num[i][f] >> 8), d[21] = (uint8_t)delay_num[i][f], d[22] = (uint8_t)(delay_den[i][f] >> 8), d[23] = (uint8_t)delay_den[i][f];
            d[24] = kPngDisposeNone, d[25] = kPngBlendSource;
            return put_chunk(to, "fcTL", d, 26);
        };
        // signature, IHDR, the caller's chunks, PLTE, tRNS, acTL and frame 0's fcTL: host bytes, placed by a copy span
        uint8_t *hd = job.blob + b;
        memcpy(hd, sig, 8);
        uint8_t ih[13];
        png_put_be32(ih, (uint32_t)width[i]), png_put_be32(ih + 4, (uint32_t)height[i]);
        ih[8] = (uint8_t)ch[(size_t)i].bd, ih[9] = (uint8_t)ch[(size_t)i].ct, ih[10] = 0, ih[11] = 0, ih[12] = (uint8_t)(interlace ? interlace[i] : 0);
        int64_t head = 8 + put_chunk(hd + 8, "IHDR", ih, 13);
        if (!xs.empty()) memcpy(hd + head, xs.data(), xs.size());
        head += (int64_t)xs.size();
        if (n_frames[i] > 1) {
            uint8_t ac[8];
            png_put_be32(ac, (uint32_t)n_frames[i]), png_put_be32(ac + 4, (uint32_t)n_plays[i]);
            head += put_chunk(hd + head, "acTL", ac, 8);
            head += put_fctl(hd + head, 0);
        }
        job.spans[k++] = Crc32Span{job.d_blob + b, o, nullptr, head, 0xFFFFFFFFu, 0, 0, 0};
        b += (size_t)head;
        int64_t pos = head;
        for (int f = 0; f < n_frames[i]; f++) {
            const size_t j = (size_t)fr0[(size_t)i] + (size_t)f;
            if (f > 0) {
                const int64_t len = put_fctl(job.blob + b, f);
                job.spans[k++] = Crc32Span{job.d_blob + b, o + pos, nullptr, len, 0xFFFFFFFFu, 0, 0, 0};
                b += (size_t)len, pos += len;
            }
            int64_t step = 0, zat = 0;
            (void)png_anim_chunks(f_zlen[j], idat_chunk_bytes, f > 0, &step);
            const int64_t zl = f_zlen[j];
            do {
                const int64_t len = std::min(step, zl - zat);
                const uint8_t *src = (const uint8_t *)f_zs[j] + zat;
                if (f == 0) {
                    job.spans[k++] = Crc32Span{src, o + pos + 8, o + pos, len, idat_init, 0, kPngIDAT, 0};
                    pos += 12 + len;
                } else {  // fdAT: the register starts behind the type and the sequence number
                    uint8_t tp[8] = {'f', 'd', 'A', 'T'};
                    png_put_be32(tp + 4, seq);
                    job.spans[k++] = Crc32Span{src, o + pos + 12, o + pos, len, ~crc32_bytes_slow(0, tp, 8), 0, kPngfdAT, seq, 1, 0};
                    seq++, pos += 16 + len;
                }
                zat += len;
            } while (zat < zl);
        }
        uint8_t *tl = job.blob + b;
        const int64_t end = put_chunk(tl, "IEND", tl, 0);
        job.spans[k++] = Crc32Span{job.d_blob + b, o + pos, nullptr, end, 0xFFFFFFFFu, 0, 0, 0};
        b += (size_t)end;
    }
    if (!crc32_run(c, &job, s)) {
        for (int &v : st)
            if (v == ZS_OK) v = ZS_STREAM_ERROR;
        rc = ZS_STREAM_ERROR;
        return finish();
    }
    if (c->profiling) c->stage_ms[kStCrc32] = job.ms;
    return finish();
}
