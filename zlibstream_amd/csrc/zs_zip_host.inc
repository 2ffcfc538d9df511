// zs_zip_host.inc -- host side of the ZIP calls of include/zsgpu.h: whole archives from host memory decoded on the device,
// and archives written on the device from entries that lie there.  Part of zs_engine.hip's translation unit, behind
// zs_parts_host.inc and zs_wrap_host.inc: the call's gate, the staging, the raw inflate of sub-streams, the roll-up of the
// codes and the one deflate call are zs_parts.h's and zs_parts_host.inc's, the KC job runner (Crc32Job) zs_png_host.inc's;
// the container's rules are zs_zip.h's, the closing kernel zs_zip.hip's.

namespace {
static_assert(sizeof(zs_zip_info) == sizeof(ZipInfo) && offsetof(zs_zip_info, zip64) == offsetof(ZipInfo, zip64), "zs_zip_info mirrors ZipInfo");
static_assert(sizeof(zs_zip_entry) == sizeof(ZipEntry) && offsetof(zs_zip_entry, status) == offsetof(ZipEntry, status) &&
                  offsetof(zs_zip_entry, out_off) == offsetof(ZipEntry, out_off) && offsetof(zs_zip_entry, crc32) == offsetof(ZipEntry, crc32),
              "zs_zip_entry mirrors ZipEntry");
static_assert(ZS_ZIP_AUTO == kZipAuto && ZS_ZIP_STORED == kZipStored && ZS_ZIP_DEFLATED == kZipDeflated && kZipMaxLen == kCrcMaxLen, "the header's constants");
static_assert(sizeof(ZipClose) == 24, "the closing kernel's descriptors lie in the job's blob");

bool zip_put_ok(const zs_zip_put &p) {
    return p.len >= 0 && p.len <= kZipMaxLen && (p.len == 0 || p.data) && p.name && p.name_len >= 1 && p.name_len <= 65535 &&
           (p.method == ZS_ZIP_AUTO || p.method == ZS_ZIP_STORED || p.method == ZS_ZIP_DEFLATED);
}
}  // namespace

extern "C" int zs_zip_file_info(const void *file, int64_t len, zs_zip_info *info, zs_zip_entry *entries, int64_t entries_cap) {
    if (!file || !info || len < 0 || entries_cap < 0 || (entries_cap > 0 && !entries)) return ZS_STREAM_ERROR;
    ZipInfo zi;
    const int rc = zip_walk((const uint8_t *)file, len, &zi, (ZipEntry *)entries, entries_cap, nullptr);
    memcpy(info, &zi, sizeof zi);
    if (rc != kZipOk) return zip_err_status(rc);
    return entries && entries_cap < zi.n_entries ? ZS_BUF_ERROR : ZS_OK;
}

extern "C" int zs_zip_decode_files_batch(zs_ctx *c, int n, const void *const *file, const int64_t *file_len, void *const *out, const int64_t *out_cap,
                                         int64_t *out_len, int *const *entry_status, int *status, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!file || !file_len || !out || !out_cap || !out_len) return ZS_STREAM_ERROR;
    for (int i = 0; i < n; i++)
        if (!file[i] || !out[i] || file_len[i] < 0 || out_cap[i] < 0) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
    const StageLayout lay(n, file_len, kZipMaxLen);  // (a larger file fails below, for itself)
    CallGate gate(n, status);
    if (!gate.open(c, hip_stream, out_len)) return ZS_STREAM_ERROR;
    hipStream_t s = gate.s;
    PartCodes pc(gate.st);
    uint8_t *d_files = nullptr;
    if (const int rc = stage_files(c, lay, file, file_len, s, &d_files)) return gate.fail_all(rc);
    // ---- the walk: every file's directory, every entry's place
    struct Ref {
        int file, entry;
    };
    std::vector<std::vector<ZipEntry>> ents((size_t)n);
    std::vector<Ref> inflated, stored;
    for (int i = 0; i < n; i++) {
        if (file_len[i] > kZipMaxLen) {
            pc.fail_file(i, ZS_DATA_ERROR, "the file is above 2 GiB - 1 KiB");
            continue;
        }
        const uint8_t *f = (const uint8_t *)file[i];
        ZipInfo zi;
        int rc = zip_find_end(f, file_len[i], &zi);
        std::vector<ZipEntry> &E = ents[(size_t)i];
        std::vector<uint8_t> errs;
        if (rc == kZipOk) {
            E.resize((size_t)zi.n_entries), errs.resize((size_t)zi.n_entries);
            rc = zip_walk(f, file_len[i], &zi, E.data(), zi.n_entries, errs.data());
        }
        if (rc == kZipOk) out_len[i] = zi.total_len;
        if (rc != kZipOk) pc.fail_file(i, zip_err_status(rc), zip_err_message(rc));
        else if (zi.total_len > kZipMaxLen) pc.fail_file(i, ZS_DATA_ERROR, "the entries are above 2 GiB - 1 KiB");
        else if (out_cap[i] < zi.total_len) pc.fail_file(i, ZS_BUF_ERROR, "buffer error");
        if (gate.st[(size_t)i] != ZS_OK) {
            E.clear();
            continue;
        }
        pc.open_parts(i, E.size());
        for (size_t e = 0; e < E.size(); e++) {
            if (E[e].status != ZS_OK) pc.fail_part(i, (int64_t)e, E[e].status, zip_err_message(errs[e]));
            else (E[e].method == kZipDeflated ? inflated : stored).push_back(Ref{i, (int)e});
        }
    }
    const std::string before = c->err;
    // ---- one raw inflate over all deflated entries, each into exactly the room that the directory's length gives it.  A
    // stream that ends in front of comp_len is accepted (what lies behind it is nobody's)
    std::vector<InfPart> parts;
    for (const Ref &r : inflated) {
        const ZipEntry &e = ents[(size_t)r.file][(size_t)r.entry];
        parts.push_back(InfPart{lay.at[(size_t)r.file] + (size_t)e.body_off, e.comp_len, (uint8_t *)out[r.file] + e.out_off, e.len, 0});
    }
    std::vector<InfResult> res;
    if (!inflate_parts(c, d_files, parts, s, &res)) return gate.fail_all(ZS_STREAM_ERROR);
    // ---- one KC job: a stored entry's body copied into place under its CRC-32, an inflated entry's output under its own
    std::vector<Ref> checked = stored;
    const size_t n_stored = checked.size();
    for (size_t j = 0; j < inflated.size(); j++) {
        const Ref &r = inflated[j];
        const PartVerdict v = part_verdict(res[j].status, res[j].msg, res[j].out_len, 0, 0, kLenExact, parts[j].out_cap);
        if (v.cls == kPartFailed) pc.fail_part(r.file, r.entry, v.code, inf_message(v.msg));
        else checked.push_back(r);
    }
    if (!checked.empty()) {
        Crc32Job job;
        bool no_memory = false;
        if (!crc32_begin(c, (int)checked.size(), 0, &job, &no_memory)) return gate.fail_all(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
        for (size_t k = 0; k < checked.size(); k++) {
            const Ref &r = checked[k];
            const ZipEntry &e = ents[(size_t)r.file][(size_t)r.entry];
            uint8_t *place = (uint8_t *)out[r.file] + e.out_off;
            if (k < n_stored) job.spans[k] = Crc32Span{d_files + lay.at[(size_t)r.file] + (size_t)e.body_off, e.len ? place : nullptr, nullptr, e.len, 0xFFFFFFFFu, 0, 0, 0};
            else job.spans[k] = Crc32Span{place, nullptr, nullptr, e.len, 0xFFFFFFFFu, 0, 0, 0};
        }
        if (!crc32_run(c, &job, s)) return gate.fail_all(ZS_STREAM_ERROR);
        png_set_stage(c, kStCrc32, job.ms);
        for (size_t k = 0; k < checked.size(); k++) {
            const Ref &r = checked[k];
            if (job.crc[k] != ents[(size_t)r.file][(size_t)r.entry].crc32) pc.fail_part(r.file, r.entry, ZS_DATA_ERROR, inf_message(kInfBadCheck));
        }
    }
    return gate.finish(pc.roll_up("file", "entry", entry_status, before, &c->err));
}

extern "C" int64_t zs_zip_bound(const zs_zip_put *entries, int n_entries) {
    if (n_entries < 0 || n_entries > 65535 || (n_entries > 0 && !entries)) return -1;
    int64_t sum = 0;
    for (int j = 0; j < n_entries; j++) {
        if (!zip_put_ok(entries[j])) return -1;
        sum += zip_entry_bound(zip_body_bound(entries[j].len, entries[j].method, zs_deflate_bound(entries[j].len)), entries[j].name_len);
    }
    const int64_t b = zip_bound(sum);
    return b > 0xFFFFFFFFll ? -1 : b;  // (an archive whose offsets need ZIP64, which is not written)
}

extern "C" int zs_zip_encode_batch_device(zs_ctx *c, int n, const zs_zip_put *const *entries, const int *n_entries, void *const *out, const int64_t *out_cap,
                                          int64_t *out_len, int *status, int level, int strategy, int hash_variant, void *hip_stream) {
    if (!c || n < 0) return ZS_STREAM_ERROR;
    if (n == 0) return ZS_OK;
    if (!entries || !n_entries || !out || !out_cap || !out_len) return ZS_STREAM_ERROR;
    struct Item {
        int archive;
        const zs_zip_put *put;
        int z;             // its stream of the deflate call, -1: none (forced stored, or empty)
        int method;        // as written
        int64_t comp_len;  // the body as written
        int64_t local_off;
    };
    std::vector<Item> items;
    std::vector<const void *> zin;
    std::vector<int64_t> zin_len, zcap;
    for (int i = 0; i < n; i++) {
        if (!out[i] || out_cap[i] < 0 || zs_zip_bound(entries[i], n_entries[i]) < 0) {
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
        for (int j = 0; j < n_entries[i]; j++) {
            const zs_zip_put *p = entries[i] + j;
            Item it{i, p, -1, ZS_ZIP_STORED, p->len, 0};
            if (p->method != ZS_ZIP_STORED && p->len > 0) {
                it.z = (int)zin.size();
                zin.push_back(p->data), zin_len.push_back(p->len), zcap.push_back(zs_deflate_bound(p->len));
            }
            items.push_back(it);
        }
    }
    CallGate gate(n, status);
    if (!gate.open(c, hip_stream, out_len)) return ZS_STREAM_ERROR;
    hipStream_t s = gate.s;
    std::vector<int> &st = gate.st;
    // ---- one deflate call over every entry that may be written deflated, into a buffer of the context
    std::vector<void *> zs_out;
    std::vector<int64_t> zlen;
    if (const int zrc = deflate_parts(c, c->png[kBufZipZs], (int)zin.size(), zin.data(), zin_len.data(), zcap.data(), level, strategy, hash_variant, s, &zs_out, &zlen))
        return gate.fail_all(zrc);
    // ---- the layout: stored or deflated per entry, every archive's length, which archives fit
    std::vector<int64_t> cd_off((size_t)n, 0), cd_len((size_t)n, 0);
    for (Item &it : items) {
        const zs_zip_put &p = *it.put;
        if (it.z >= 0) {
            const int64_t raw = zlen[(size_t)it.z] - 6;
            if (p.method == ZS_ZIP_DEFLATED || raw < p.len) it.method = ZS_ZIP_DEFLATED, it.comp_len = raw;
        }
        it.local_off = cd_off[(size_t)it.archive];
        cd_off[(size_t)it.archive] += kZipLocalBytes + p.name_len + it.comp_len;
        cd_len[(size_t)it.archive] += kZipCentralBytes + p.name_len;
    }
    int rc = ZS_OK;
    size_t fit_items = 0, fit_spans = 0, head_bytes = 0;
    for (int i = 0; i < n; i++) out_len[i] = cd_off[(size_t)i] + cd_len[(size_t)i] + kZipEndBytes;
    if (mark_fit(st, out_len, out_cap, &rc, &c->err) == 0) return gate.finish(rc);
    for (int i = 0; i < n; i++)
        if (st[(size_t)i] == ZS_OK) head_bytes += (size_t)cd_len[(size_t)i] + kZipEndBytes, fit_spans++;
    for (const Item &it : items)
        if (st[(size_t)it.archive] == ZS_OK) fit_items++, fit_spans += it.method == ZS_ZIP_DEFLATED ? 3 : 2, head_bytes += (size_t)kZipLocalBytes + (size_t)it.put->name_len;
    // ---- one KC job.  Per entry: the local header and name (host bytes in the job's blob) copied into place; the body --
    // bytes [2, L - 4) of the zlib stream, or the data itself with its CRC-32 taken by the same span --; for a deflated entry a
    // CRC-only span over the data.  Per archive: the central directory and the end record, host bytes again.  The blob: the
    // closing kernel's descriptors, then those bytes.
    const size_t b_close = sizeof(ZipClose) * fit_items;
    Crc32Job job;
    bool no_memory = false;
    if (!crc32_begin(c, (int)fit_spans, b_close + head_bytes, &job, &no_memory)) return gate.fail_live(no_memory ? ZS_MEM_ERROR : ZS_STREAM_ERROR);
    ZipClose *closes = (ZipClose *)job.blob;
    uint8_t *hb = job.blob + b_close;  // the next host bytes
    int sp = 0;
    size_t k_item = 0, first = 0;
    for (int i = 0; i < n; i++) {
        size_t last = first;
        while (last < items.size() && items[last].archive == i) last++;
        if (st[(size_t)i] == ZS_OK) {
            uint8_t *o = (uint8_t *)out[i];
            uint8_t *cd = hb;  // the directory is built while the entries go by, its span follows them
            hb += (size_t)cd_len[(size_t)i] + kZipEndBytes;
            uint8_t *rec = cd;
            for (size_t q = first; q < last; q++) {
                const Item &it = items[q];
                const zs_zip_put &p = *it.put;
                const uint32_t nl = (uint32_t)p.name_len;
                zip_put_local(hb, it.method, p.utf8, p.dos_time, p.dos_date, (uint32_t)it.comp_len, (uint32_t)p.len, nl);
                memcpy(hb + kZipLocalBytes, p.name, nl);
                job.spans[sp++] = Crc32Span{job.d_blob + (hb - job.blob), o + it.local_off, nullptr, kZipLocalBytes + (int64_t)nl, 0xFFFFFFFFu, 0, 0, 0};
                hb += kZipLocalBytes + nl;
                uint8_t *body = o + it.local_off + kZipLocalBytes + nl;
                int crc_span;
                if (it.method == ZS_ZIP_DEFLATED) {
                    job.spans[sp++] = Crc32Span{(const uint8_t *)zs_out[(size_t)it.z] + 2, body, nullptr, it.comp_len, 0xFFFFFFFFu, 0, 0, 0};
                    crc_span = sp;
                    job.spans[sp++] = Crc32Span{(const uint8_t *)p.data, nullptr, nullptr, p.len, 0xFFFFFFFFu, 0, 0, 0};
                } else {
                    crc_span = sp;  // (an empty entry: a span without bytes, whose CRC-32 is 0)
                    job.spans[sp++] = Crc32Span{p.len ? (const uint8_t *)p.data : job.d_blob, p.len ? body : nullptr, nullptr, p.len, 0xFFFFFFFFu, 0, 0, 0};
                }
                zip_put_central(rec, it.method, p.utf8, p.dos_time, p.dos_date, (uint32_t)it.comp_len, (uint32_t)p.len, nl, p.external_attr, (uint32_t)it.local_off);
                memcpy(rec + kZipCentralBytes, p.name, nl);
                closes[k_item++] = ZipClose{o + it.local_off + 14, o + cd_off[(size_t)i] + (rec - cd) + 16, (uint32_t)crc_span, 0};
                rec += kZipCentralBytes + nl;
            }
            zip_put_eocd(rec, (uint32_t)(last - first), (uint32_t)cd_len[(size_t)i], (uint32_t)cd_off[(size_t)i]);
            job.spans[sp++] = Crc32Span{job.d_blob + (cd - job.blob), o + cd_off[(size_t)i], nullptr, cd_len[(size_t)i] + kZipEndBytes, 0xFFFFFFFFu, 0, 0, 0};
        }
        first = last;
    }
    // ---- KZ behind KC's finishing launch and in front of its one wait: the CRCs never leave the device
    const int n_close = (int)fit_items;
    const std::function<bool(const uint32_t *)> close = [&](const uint32_t *d_crc) {
        hipLaunchKernelGGL(zs_zip_close_kernel, dim3((unsigned)((n_close + 63) / 64)), dim3(64), 0, s, (const ZipClose *)job.d_blob, n_close, d_crc);
        return hipGetLastError() == hipSuccess;
    };
    if (!crc32_run(c, &job, s, n_close ? &close : nullptr)) return gate.fail_live(ZS_STREAM_ERROR);
    if (c->profiling) c->stage_ms[kStCrc32] = job.ms;
    return gate.finish(rc);
}
