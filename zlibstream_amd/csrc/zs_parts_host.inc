// zs_parts_host.inc -- the plumbing that the container calls share, beside the rules of zs_parts.h: a call's gate and status
// vector, the one staging of n host files, the raw inflate of sub-streams that lie inside the staged files, the Adler-32
// compare behind it, and the one deflate call of an encode.  Part of zs_engine.hip's translation unit, behind
// zs_png_host.inc (ensure, run_inflate, device_adlers are the engine's) and in front of zs_wrap_host.inc and the container
// files, which keep their walks, routes, span lists and kernel runs.

#include "zs_parts.h"

namespace {
static_assert((int)kPartBadMethod == kInfBadMethod && (int)kPartBadWindow == kInfBadWindow && (int)kPartBadHeaderCheck == kInfBadHeaderCheck &&
                  (int)kPartNeedDict == kInfNeedDict && (int)kPartTruncated == kInfTruncated && (int)kPartOutputFull == kInfOutputFull && (int)kPartBadLength == kInfBadLength,
              "zs_parts.h names InfMsg's numbers");

// A call over n files or outputs: its stream and its status vector, which every way out of the call copies to the caller.
struct CallGate {
    hipStream_t s = nullptr;
    int *status;
    std::vector<int> st;
    int *also_out = nullptr;  // a second per-file result that leaves with the codes (the gzip files call's member counts)
    const std::vector<int> *also = nullptr;
    CallGate(int n, int *status_) : status(status_), st((size_t)n, ZS_OK) {}
    // the device and the stream; out_len (may be null) is zeroed.  False: the call ends with ZS_STREAM_ERROR, nothing written
    bool open(zs_ctx *c, void *hip_stream, int64_t *out_len) {
        if (hipSetDevice(c->device) != hipSuccess) return false;
        s = hip_stream ? (hipStream_t)hip_stream : c->stream;
        if (out_len) std::fill(out_len, out_len + st.size(), (int64_t)0);
        return true;
    }
    int finish(int rc) {
        if (status) memcpy(status, st.data(), sizeof(int) * st.size());
        if (also_out) memcpy(also_out, also->data(), sizeof(int) * st.size());
        return rc;
    }
    int fail_all(int rc) {
        std::fill(st.begin(), st.end(), rc);
        return finish(rc);
    }
    int fail_live(int rc) {  // a job over the outputs that fit failed
        zs::fail_live(st, rc);
        return finish(rc);
    }
};

// The n items of `lay` from host memory into png[kBufWrapFiles], one copy and one wait: ZS_OK and the buffer, ZS_MEM_ERROR,
// or ZS_STREAM_ERROR.  The copy goes through the context's pinned buffer, which the inflate calls behind this use for their
// own descriptors: the wait is here, before any of them takes it.
int stage_files(zs_ctx *c, const StageLayout &lay, const void *const *ptr, const int64_t *len, hipStream_t s, uint8_t **d_files) {
    if (!ensure(c, c->png[kBufWrapFiles], lay.total + 256) || !ensure_pinned(c, lay.total + 256)) return ZS_MEM_ERROR;
    for (size_t i = 0; i < lay.at.size(); i++)
        if (lay.staged(len[i])) memcpy((uint8_t *)c->pinned + lay.at[i], ptr[i], (size_t)len[i]);
    *d_files = (uint8_t *)c->png[kBufWrapFiles].p;
    if (lay.total && hipMemcpyAsync(*d_files, c->pinned, lay.total, hipMemcpyHostToDevice, s) != hipSuccess) return ZS_STREAM_ERROR;
    return hipStreamSynchronize(s) == hipSuccess ? ZS_OK : ZS_STREAM_ERROR;
}

// A sub-stream of the staged files and where it inflates to; skip: 2 for a zlib stream whose header the host has checked
struct InfPart {
    size_t pos;  // in the staged buffer
    int64_t comp_len;
    void *out;
    int64_t out_cap;
    int skip;
};
struct InfResult {
    int status = ZS_STREAM_ERROR, msg = 0;
    int64_t out_len = 0, used = 0;  // used: from the part's first byte
};
// One raw inflate over the parts (zs_parts.h, sub_stream: 16-byte-aligned pointers, the rest in InfWrap::body_off).  False:
// the call itself failed and its message stands; else every part's result, for part_verdict.
bool inflate_parts(zs_ctx *c, const uint8_t *d_files, const std::vector<InfPart> &parts, hipStream_t s, std::vector<InfResult> *res) {
    const size_t m = parts.size();
    res->assign(m, InfResult());
    if (m == 0) return true;
    std::vector<const void *> sin(m);
    std::vector<void *> sout(m);
    std::vector<int64_t> slen(m), scap(m), olen(m, 0), used(m, 0);
    std::vector<int32_t> body(m);
    std::vector<int> sst(m, ZS_STREAM_ERROR), smsg(m, 0);
    for (size_t j = 0; j < m; j++) {
        const SubStream ss = sub_stream(parts[j].pos, parts[j].comp_len, parts[j].skip);  // (d_files and every file's place are 256-byte aligned)
        sin[j] = d_files + ss.base, slen[j] = ss.in_len, body[j] = ss.body_off;
        sout[j] = parts[j].out, scap[j] = parts[j].out_cap;
    }
    InfWrap wr;
    wr.body_off = body.data(), wr.msg = smsg.data(), wr.in_used = used.data();
    (void)run_inflate(c, (int)m, sin.data(), slen.data(), sout.data(), scap.data(), olen.data(), sst.data(), s, nullptr, wr);
    bool call_ok = true;
    for (size_t j = 0; j < m; j++) {
        (*res)[j] = InfResult{sst[j], smsg[j], olen[j], used[j] - (body[j] - parts[j].skip)};
        if (sst[j] == ZS_STREAM_ERROR || sst[j] == ZS_OK) call_ok = false;
    }
    return call_ok;
}

// The Adler-32 of every buffer in one launch, against the four big-endian bytes at its trailer (host memory).  False: the
// launch failed; else same[a].
bool check_adlers(zs_ctx *c, const std::vector<const void *> &buf, const std::vector<int64_t> &len, const std::vector<const uint8_t *> &trailer, hipStream_t s,
                  std::vector<bool> *same) {
    same->assign(buf.size(), false);
    if (buf.empty()) return true;
    std::vector<uint32_t> ads(buf.size(), 0);
    if (!device_adlers(c, (int)buf.size(), buf.data(), len.data(), nullptr, ads.data(), nullptr, s)) return false;
    for (size_t a = 0; a < buf.size(); a++) {
        const uint8_t *t = trailer[a];
        (*same)[a] = ((uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | t[3]) == ads[a];
    }
    return true;
}

// One deflate call over m parts into `buf` of the context, every stream at a multiple of 256: (*zout)[k] and (*zlen)[k].
// ZS_OK, or the code that the whole call fails with.
int deflate_parts(zs_ctx *c, DevBuf &buf, int m, const void *const *zin, const int64_t *zin_len, const int64_t *zcap, int level, int strategy, int hash_variant, hipStream_t s,
                  std::vector<void *> *zout, std::vector<int64_t> *zlen) {
    zout->assign((size_t)m, nullptr), zlen->assign((size_t)m, 0);
    if (m == 0) return ZS_OK;
    size_t z_total = 0;
    for (int k = 0; k < m; k++) z_total += pad256((size_t)zcap[k]);
    if (!ensure(c, buf, z_total + 256)) return ZS_MEM_ERROR;
    size_t at = 0;
    for (int k = 0; k < m; k++) (*zout)[(size_t)k] = (uint8_t *)buf.p + at, at += pad256((size_t)zcap[k]);
    std::vector<int> zst((size_t)m, ZS_STREAM_ERROR);
    const int zrc = zs_deflate_batch_device(c, m, zin, zin_len, zout->data(), zcap, zlen->data(), zst.data(), level, strategy, hash_variant, (void *)s);
    if (zrc != ZS_OK) return zrc;
    for (int k = 0; k < m; k++)
        if ((*zlen)[(size_t)k] < 6) {  // (no zlib stream is that short)
            c->err = "stream error";
            return ZS_STREAM_ERROR;
        }
    return ZS_OK;
}
}  // namespace
