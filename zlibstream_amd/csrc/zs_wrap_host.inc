// zs_wrap_host.inc -- host side of the container calls of include/zsgpu.h (raw deflate and gzip beside zlib): gzip members
// through the inflate paths, the framing launch behind a deflate call, and gzip files from host memory.  Part of
// zs_engine.hip's translation unit, behind zs_png_host.inc, whose KC job runner (Crc32Job) it uses, and zs_parts_host.inc,
// whose gate, staging and file codes the gzip files call takes; the rules of a gzip header are zs_gzip.h's, the two small
// kernels zs_gzip.hip's.  zs_deflate_wrap_batch_device keeps its own deflate call and layout: a stream of its that comes out
// too short fails for itself, where deflate_parts fails the call.

namespace {

// a header's error in inflate's terms
void gz_err_code(int gz_err, int *status, int *msg) {
    switch (gz_err) {
    case kGzTruncated: *status = ZS_BUF_ERROR, *msg = kInfTruncated; break;
    case kGzBadMagic: *status = ZS_DATA_ERROR, *msg = kInfBadHeaderCheck; break;
    case kGzBadMethod: *status = ZS_DATA_ERROR, *msg = kInfBadMethod; break;
    case kGzBadFlags: *status = ZS_DATA_ERROR, *msg = kInfBadFlags; break;
    default: *status = ZS_DATA_ERROR, *msg = kInfBadHeaderCrc; break;
    }
}

uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

bool inflate_gzip_members(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out, const int64_t *out_cap,
                          int64_t *out_len, int64_t *in_used, int *status, int *msg_out, hipStream_t s) {
    std::vector<int> msg((size_t)n, 0);
    auto leave = [&](bool ok) {
        // the call's message is its first failing member's, whichever step refused it
        for (int i = 0; i < n; i++)
            if (status[i] != ZS_STREAM_END) {
                if (msg[(size_t)i] > 0) c->err = inf_message(msg[(size_t)i]);
                break;
            }
        if (msg_out) memcpy(msg_out, msg.data(), sizeof(int) * (size_t)n);
        return ok;
    };
    // ---- 1. the headers: descriptors up, one lane per member, 16 bytes per member back
    const size_t b_desc = sizeof(GzMember) * (size_t)n, b_head = sizeof(GzHead) * (size_t)n;
    if (!ensure(c, c->png[kBufWrapHead], b_desc + b_head) || !ensure_pinned(c, b_desc + b_head)) return false;
    GzMember *hm = (GzMember *)c->pinned;
    const GzHead *hh = (const GzHead *)((uint8_t *)c->pinned + b_desc);
    for (int i = 0; i < n; i++) hm[i] = GzMember{(const uint8_t *)in[i], in_len[i]};
    GzMember *d_m = (GzMember *)c->png[kBufWrapHead].p;
    GzHead *d_h = (GzHead *)((uint8_t *)c->png[kBufWrapHead].p + b_desc);
    ZS_HIP(c, hipMemcpyAsync(d_m, hm, b_desc, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(zs_gzip_header_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (const GzMember *)d_m, n, d_h);
    ZS_HIP(c, hipGetLastError());
    ZS_HIP(c, hipMemcpyAsync((void *)hh, d_h, b_head, hipMemcpyDeviceToHost, s));
    ZS_HIP(c, hipStreamSynchronize(s));
    std::vector<int> idx;
    std::vector<int32_t> body;
    for (int i = 0; i < n; i++) {
        out_len[i] = 0;
        if (in_used) in_used[i] = 0;
        if (hh[i].err != kGzOk) gz_err_code(hh[i].err, &status[i], &msg[(size_t)i]);
        else idx.push_back(i), body.push_back(hh[i].body_off);
    }
    const int m = (int)idx.size();
    if (m == 0) return leave(false);
    // ---- 2. raw inflate from the bodies' offsets (the pinned buffer is the inflate call's from here on)
    std::vector<const void *> sin((size_t)m);
    std::vector<void *> sout((size_t)m);
    std::vector<int64_t> slen((size_t)m), scap((size_t)m), solen((size_t)m, 0), sused((size_t)m, 0);
    std::vector<int> sst((size_t)m, ZS_STREAM_ERROR), smsg((size_t)m, 0);
    for (int j = 0; j < m; j++) {
        const int i = idx[(size_t)j];
        sin[(size_t)j] = in[i], sout[(size_t)j] = out[i], slen[(size_t)j] = in_len[i], scap[(size_t)j] = out_cap[i];
    }
    InfWrap wr;
    wr.body_off = body.data(), wr.in_used = sused.data(), wr.msg = smsg.data();
    const bool inf_ok = run_inflate(c, m, sin.data(), slen.data(), sout.data(), scap.data(), solen.data(), sst.data(), s, nullptr, wr);
    bool infra = false;  // the inflate call itself failed (a HIP error, no memory): its message stands
    std::vector<int> fin;  // members whose body decoded and whose trailer is all there
    for (int j = 0; j < m; j++) {
        const int i = idx[(size_t)j];
        status[i] = sst[(size_t)j], msg[(size_t)i] = smsg[(size_t)j], out_len[i] = solen[(size_t)j];
        if (sst[(size_t)j] == ZS_STREAM_ERROR || sst[(size_t)j] == ZS_OK) infra = true, status[i] = ZS_STREAM_ERROR;
        if (sst[(size_t)j] != ZS_STREAM_END) continue;
        if (sused[(size_t)j] + kGzipTrailBytes > in_len[i]) {  // the member ends inside its trailer
            status[i] = ZS_BUF_ERROR, msg[(size_t)i] = kInfTruncated;
            continue;
        }
        fin.push_back(j);
    }
    if (!inf_ok && infra) return false;
    if (fin.empty()) return leave(false);
    // ---- 3. KC over the outputs, and the trailers gathered by its span copy: one copy back for all of them
    const int k = (int)fin.size();
    if (!ensure(c, c->png[kBufWrapGather], (size_t)kGzipTrailBytes * (size_t)k + 16)) return false;
    Crc32Job job;
    bool no_memory = false;
    if (!crc32_begin(c, 2 * k, 0, &job, &no_memory)) return false;
    uint8_t *d_gather = (uint8_t *)c->png[kBufWrapGather].p;
    for (int t = 0; t < k; t++) {
        const int j = fin[(size_t)t], i = idx[(size_t)j];
        job.spans[2 * t] = Crc32Span{(const uint8_t *)out[i], nullptr, nullptr, solen[(size_t)j], 0xFFFFFFFFu, 0, 0, 0};
        job.spans[2 * t + 1] = Crc32Span{(const uint8_t *)in[i] + sused[(size_t)j], d_gather + (size_t)kGzipTrailBytes * (size_t)t, nullptr, kGzipTrailBytes,
                                         0xFFFFFFFFu, 0, 0, 0};
    }
    std::vector<uint8_t> trail((size_t)kGzipTrailBytes * (size_t)k);
    const std::function<bool(const uint32_t *)> fetch = [&](const uint32_t *) {
        return hipMemcpyAsync(trail.data(), d_gather, trail.size(), hipMemcpyDeviceToHost, s) == hipSuccess;
    };
    if (!crc32_run(c, &job, s, &fetch)) return false;
    png_set_stage(c, kStCrc32, job.ms);
    // ---- 4. the compare (inflate.c CHECK, LENGTH)
    bool all = inf_ok && m == n;
    for (int t = 0; t < k; t++) {
        const int j = fin[(size_t)t], i = idx[(size_t)j];
        const uint8_t *tr = trail.data() + (size_t)kGzipTrailBytes * (size_t)t;
        if (le32(tr) != job.crc[2 * t]) status[i] = ZS_DATA_ERROR, msg[(size_t)i] = kInfBadCheck, all = false;
        else if (le32(tr + 4) != (uint32_t)solen[(size_t)j]) status[i] = ZS_DATA_ERROR, msg[(size_t)i] = kInfBadLength, all = false;
        else if (in_used) in_used[i] = sused[(size_t)j] + kGzipTrailBytes;
    }
    if ((int)fin.size() != m) all = false;
    return leave(all);
}

}  // namespace

extern "C" int64_t zs_wrap_bound(int64_t n, int wrap) {
    if (n < 0 || wrap < ZS_WRAP_ZLIB || wrap > ZS_WRAP_GZIP) return -1;
    return zs_deflate_bound(n) - 6 + wrap_head_bytes(wrap) + wrap_tail_bytes(wrap);
}

extern "C" int zs_deflate_wrap_batch_device(zs_ctx *c, int n, const void *const *in, const int64_t *in_len, void *const *out, const int64_t *out_cap,
                                            int64_t *out_len, int *status, int level, int strategy, int hash_variant, int wrap, void *hip_stream) {
    if (wrap == ZS_WRAP_ZLIB) return zs_deflate_batch_device(c, n, in, in_len, out, out_cap, out_len, status, level, strategy, hash_variant, hip_stream);
    if (!c || n < 0 || (wrap != ZS_WRAP_RAW && wrap != ZS_WRAP_GZIP)) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!in || !in_len || !out || !out_cap || !out_len) return ZS_STREAM_ERROR;
    size_t z_total = 0;
    std::vector<int64_t> zcap((size_t)n), zlen((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        if (in_len[i] < 0 || in_len[i] > kCrcMaxLen || out_cap[i] < 0 || !out[i] || (in_len[i] > 0 && !in[i])) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        zcap[(size_t)i] = zs_deflate_bound(in_len[i]);
        z_total += pad256((size_t)zcap[(size_t)i]);
    }
    if (hipSetDevice(c->device) != hipSuccess) return ZS_STREAM_ERROR;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    std::vector<int> st((size_t)n, ZS_STREAM_ERROR);
    auto finish = [&](int rc) {
        if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
        return rc;
    };
    if (!ensure(c, c->png[kBufWrapZs], z_total + 256)) {
        std::fill(st.begin(), st.end(), (int)ZS_MEM_ERROR);
        return finish(ZS_MEM_ERROR);
    }
    std::vector<void *> zs_out((size_t)n);
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        zs_out[(size_t)i] = (uint8_t *)c->png[kBufWrapZs].p + at;
        at += pad256((size_t)zcap[(size_t)i]);
    }
    const int zrc = zs_deflate_batch_device(c, n, in, in_len, zs_out.data(), zcap.data(), zlen.data(), st.data(), level, strategy, hash_variant, (void *)s);
    if (zrc != ZS_OK) {
        for (int i = 0; i < n; i++) out_len[i] = 0;
        return finish(zrc);
    }
    // ---- the layout: which streams fit; a stream that does not is left out of the framing launch
    const int head = wrap_head_bytes(wrap), tail = wrap_tail_bytes(wrap);
    const bool gz = wrap == ZS_WRAP_GZIP;
    int rc = ZS_OK, n_fit = 0;
    for (int i = 0; i < n; i++) {
        out_len[i] = head + (zlen[(size_t)i] - 6) + tail;
        if (zlen[(size_t)i] < 6) {  // (no zlib stream is that short)
            st[(size_t)i] = ZS_STREAM_ERROR, out_len[i] = 0;
            if (rc == ZS_OK) rc = ZS_STREAM_ERROR, c->err = "stream error";
        } else if (out_cap[i] < out_len[i]) {
            st[(size_t)i] = ZS_BUF_ERROR;
            if (rc == ZS_OK) rc = ZS_BUF_ERROR, c->err = "buffer error";
        } else {
            n_fit++;
        }
    }
    if (n_fit == 0) return finish(rc);
    // spans per stream: the body; for gzip also the ten header bytes (host bytes in the job's blob) and the input, whose
    // CRC-32 the trailer kernel puts behind the body.  The blob: the trailers' descriptors, then the headers.
    const int per = gz ? 3 : 1;
    const size_t b_trail = gz ? sizeof(GzTrail) * (size_t)n_fit : 0;
    Crc32Job job;
    bool no_memory = false;
    if (!crc32_begin(c, per * n_fit, b_trail + (gz ? (size_t)kGzipHeadBytes * (size_t)n_fit : 0), &job, &no_memory)) {
        for (int i = 0; i < n; i++)
            if (st[(size_t)i] == ZS_OK) st[(size_t)i] = no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR;
        return finish(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    }
    GzTrail *trails = (GzTrail *)job.blob;
    int k = 0;
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        uint8_t *o = (uint8_t *)out[i];
        const int64_t body = zlen[(size_t)i] - 6;
        job.spans[per * k] = Crc32Span{(const uint8_t *)zs_out[(size_t)i] + 2, o + head, nullptr, body, 0xFFFFFFFFu, 0, 0, 0};
        if (gz) {
            uint8_t *hd = job.blob + b_trail + (size_t)kGzipHeadBytes * (size_t)k;
            gzip_put_header(hd, level);
            job.spans[per * k + 1] = Crc32Span{job.d_blob + (hd - job.blob), o, nullptr, kGzipHeadBytes, 0xFFFFFFFFu, 0, 0, 0};
            job.spans[per * k + 2] = Crc32Span{(const uint8_t *)in[i], nullptr, nullptr, in_len[i], 0xFFFFFFFFu, 0, 0, 0};
            trails[k] = GzTrail{o + head + body, (uint32_t)(per * k + 2), (uint32_t)(uint64_t)in_len[i]};
        }
        k++;
    }
    const std::function<bool(const uint32_t *)> close = [&](const uint32_t *d_crc) {
        hipLaunchKernelGGL(zs_gzip_trailer_kernel, dim3((unsigned)((n_fit + 63) / 64)), dim3(64), 0, s, (const GzTrail *)job.d_blob, n_fit, d_crc);
        return hipGetLastError() == hipSuccess;
    };
    if (!crc32_run(c, &job, s, gz ? &close : nullptr)) return finish(ZS_STREAM_ERROR);
    if (c->profiling) c->stage_ms[kStCrc32] = job.ms;
    return finish(rc);
}

// ------------------------------------------------------------------ gzip files
namespace {

struct GzFileMember {
    int64_t off, size;  // in the file
    uint32_t isize;
};
bool all_zero(const uint8_t *p, int64_t from, int64_t len) {
    for (int64_t i = from; i < len; i++)
        if (p[i]) return false;
    return true;
}
// The walk over a BGZF file by its members' sizes.  ZS_OK: the members, up to the end of the file or the zero bytes behind the
// last one.  Otherwise the members in front of the place where the walk stopped, and why: ZS_BUF_ERROR -- a header or a
// member that the file ends in --, ZS_DATA_ERROR -- a header that is not gzip's (*gz_err says which rule) or has no BGZF
// subfield (kGzOk), a member too short for its own header and trailer.
int bgzf_walk(const uint8_t *f, int64_t len, std::vector<GzFileMember> *members, int *gz_err) {
    *gz_err = kGzOk;
    for (int64_t at = 0; at < len;) {
        if (!members->empty() && all_zero(f, at, len)) break;
        GzHeader h;
        const int e = gzip_parse_header(f + at, len - at, &h);
        if (e != kGzOk) {
            *gz_err = e;
            return e == kGzTruncated ? ZS_BUF_ERROR : ZS_DATA_ERROR;
        }
        if (h.member_size == 0 || h.member_size < h.body_off + kGzipTrailBytes) return ZS_DATA_ERROR;
        if (at + h.member_size > len) return ZS_BUF_ERROR;
        members->push_back(GzFileMember{at, h.member_size, le32(f + at + h.member_size - 4)});
        at += h.member_size;
    }
    return ZS_OK;
}

}  // namespace

extern "C" int zs_gzip_file_info(const void *file, int64_t len, zs_gzip_info *info) {
    if (!file || !info || len < 0) return ZS_STREAM_ERROR;
    const uint8_t *f = (const uint8_t *)file;
    GzHeader h;
    const int e = gzip_parse_header(f, len, &h);
    memset(info, 0, sizeof *info);
    info->n_members = -1, info->isize_sum = -1;
    if (e != kGzOk) return e == kGzTruncated ? ZS_BUF_ERROR : ZS_DATA_ERROR;
    info->bgzf = h.member_size != 0, info->xfl = h.xfl, info->os = h.os, info->mtime = h.mtime;
    info->name_off = h.name_off, info->name_len = h.name_len;
    if (!info->bgzf) return ZS_OK;
    std::vector<GzFileMember> members;
    int gz_err = kGzOk;
    const int rc = bgzf_walk(f, len, &members, &gz_err);
    if (rc != ZS_OK) return rc;
    info->n_members = (int64_t)members.size();
    info->isize_sum = 0;
    for (const GzFileMember &m : members) info->isize_sum += m.isize;
    return ZS_OK;
}

extern "C" int zs_gzip_decode_files_batch(zs_ctx *c, int n, const void *const *file, const int64_t *file_len, void *const *out, const int64_t *out_cap,
                                          int64_t *out_len, int *n_members, int *status, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!file || !file_len || !out || !out_cap || !out_len) return ZS_STREAM_ERROR;
    // (a file above the limit is refused for the whole call, as the header says: elsewhere such a file fails for itself)
    for (int i = 0; i < n; i++)
        if (!file[i] || !out[i] || file_len[i] < 0 || file_len[i] > kCrcMaxLen || out_cap[i] < 0 || out_cap[i] > kCrcMaxLen) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
    const StageLayout lay(n, file_len, kCrcMaxLen);
    std::vector<int> cnt((size_t)n, 0);
    CallGate gate(n, status);
    gate.also_out = n_members, gate.also = &cnt;
    if (!gate.open(c, hip_stream, out_len)) return ZS_STREAM_ERROR;
    hipStream_t s = gate.s;
    PartCodes pc(gate.st);
    uint8_t *d_files = nullptr;
    if (const int rc = stage_files(c, lay, file, file_len, s, &d_files)) return gate.fail_all(rc);
    // ---- BGZF files: every member of every file is one stream of one launch
    std::vector<bool> plain((size_t)n, true);
    {
        std::vector<const void *> in;
        std::vector<void *> o;
        std::vector<int64_t> ilen, ocap;
        std::vector<int> owner;
        for (int i = 0; i < n; i++) {
            const uint8_t *f = (const uint8_t *)file[i];
            GzHeader h;
            if (gzip_parse_header(f, file_len[i], &h) != kGzOk || h.member_size == 0) continue;  // (a bad first header: the rounds report it)
            plain[(size_t)i] = false;
            std::vector<GzFileMember> members;
            int gz_err = kGzOk, wst = ZS_OK, wmsg = 0;
            const int rc = bgzf_walk(f, file_len[i], &members, &gz_err);
            if (rc != ZS_OK) {
                if (gz_err != kGzOk) gz_err_code(gz_err, &wst, &wmsg);
                else wst = rc, wmsg = rc == ZS_BUF_ERROR ? (int)kInfTruncated : (int)kInfBadHeaderCheck;
                pc.fail_file(i, wst, inf_message(wmsg));
            }
            int64_t sum = 0;
            for (const GzFileMember &m : members) sum += m.isize;
            if (sum > out_cap[i]) {
                pc.fail_file(i, ZS_BUF_ERROR, inf_message(kInfOutputFull));
                continue;
            }
            int64_t pos = 0;
            for (const GzFileMember &m : members) {
                in.push_back(d_files + lay.at[(size_t)i] + m.off), ilen.push_back(m.size);
                o.push_back((uint8_t *)out[i] + pos), ocap.push_back((int64_t)m.isize), owner.push_back(i);
                pos += m.isize;
            }
        }
        const int m = (int)in.size();
        if (m) {
            std::vector<int64_t> olen((size_t)m, 0), used((size_t)m, 0);
            std::vector<int> mst((size_t)m, ZS_STREAM_ERROR), mmsg((size_t)m, 0);
            const std::string before = c->err;
            const bool ok = inflate_gzip_members(c, m, in.data(), ilen.data(), o.data(), ocap.data(), olen.data(), used.data(), mst.data(), mmsg.data(), s);
            std::vector<bool> closed((size_t)n, false);  // a member of the file has failed: what lies behind it does not count
            for (int j = 0; j < m; j++) {  // (a file's members stand in the file's order)
                const int i = owner[(size_t)j];
                if (mst[(size_t)j] == ZS_STREAM_ERROR) return gate.fail_all(ZS_STREAM_ERROR);  // (the call itself failed: its message stands)
                if (closed[(size_t)i]) continue;
                if (mst[(size_t)j] == ZS_STREAM_END) {
                    cnt[(size_t)i]++, out_len[i] += olen[(size_t)j];
                    continue;
                }
                // (it lies in front of whatever the walk stopped at: its reason is the file's, over the walk's.)  A body longer
                // than its ISIZE ran out of the room the ISIZE gave it (part_failure)
                int why = 0;
                closed[(size_t)i] = true;
                part_failure(mst[(size_t)j], mmsg[(size_t)j], &gate.st[(size_t)i], &why);
                pc.why[(size_t)i] = inf_message(why);
            }
            if (ok) c->err = before;
        }
    }
    // ---- the other files: round r decodes member r of every file that still has bytes
    std::vector<int64_t> pos((size_t)n, 0);
    std::vector<int> live;
    for (int i = 0; i < n; i++)
        if (plain[(size_t)i]) live.push_back(i);
    while (!live.empty()) {
        const int m = (int)live.size();
        std::vector<const void *> in((size_t)m);
        std::vector<void *> o((size_t)m);
        std::vector<int64_t> ilen((size_t)m), ocap((size_t)m), olen((size_t)m, 0), used((size_t)m, 0);
        std::vector<int> mst((size_t)m, ZS_STREAM_ERROR), mmsg((size_t)m, 0);
        for (int j = 0; j < m; j++) {
            const int i = live[(size_t)j];
            in[(size_t)j] = d_files + lay.at[(size_t)i] + pos[(size_t)i], ilen[(size_t)j] = file_len[i] - pos[(size_t)i];
            o[(size_t)j] = (uint8_t *)out[i] + out_len[i], ocap[(size_t)j] = out_cap[i] - out_len[i];
        }
        (void)inflate_gzip_members(c, m, in.data(), ilen.data(), o.data(), ocap.data(), olen.data(), used.data(), mst.data(), mmsg.data(), s);
        std::vector<int> next;
        for (int j = 0; j < m; j++) {
            const int i = live[(size_t)j];
            if (mst[(size_t)j] == ZS_STREAM_ERROR) return gate.fail_all(ZS_STREAM_ERROR);
            if (mst[(size_t)j] != ZS_STREAM_END) {
                pc.fail_file(i, mst[(size_t)j], inf_message(mmsg[(size_t)j]));
                continue;
            }
            cnt[(size_t)i]++, out_len[i] += olen[(size_t)j], pos[(size_t)i] += used[(size_t)j];
            if (pos[(size_t)i] < file_len[i] && !all_zero((const uint8_t *)file[i], pos[(size_t)i], file_len[i])) next.push_back(i);
        }
        live.swap(next);
    }
    return gate.finish(pc.first_file("file", &c->err));
}
