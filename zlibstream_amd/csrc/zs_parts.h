// zs_parts.h -- the rules that the container calls share (gzip files, ZIP, TIFF, OpenEXR, chunked arrays): how n host files
// are laid out for one upload, where a sub-stream inside an uploaded file begins for the inflate kernels, what a zlib header
// must say, what becomes of an inflated sub-stream, how the codes and messages of parts roll up into their files' and the
// call's, and which outputs of an encode call fit.  Plain C++17 without HIP: tests/cpp/test_parts.cpp runs it on the host.
// The plumbing that goes with it is zs_parts_host.inc's.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zsgpu.h"

namespace zs {

// The InfMsg numbers that these rules name (zs_inflate.hip's enum, which only a HIP compiler reads; zs_parts_host.inc
// asserts that the two agree).
enum PartMsg { kPartBadMethod = 1, kPartBadWindow = 2, kPartBadHeaderCheck = 3, kPartNeedDict = 4, kPartTruncated = 18, kPartOutputFull = 19, kPartBadLength = 23 };

inline size_t pad256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- the staging of n items in one buffer: every item at a multiple of 256; an item above `limit` takes no room (it fails
// for itself, behind the upload), one without bytes none either
struct StageLayout {
    int64_t limit;
    std::vector<size_t> at;
    size_t total = 0;
    explicit StageLayout(int64_t limit_) : limit(limit_) {}
    StageLayout(int n, const int64_t *len, int64_t limit_) : limit(limit_) {
        at.reserve((size_t)n);
        for (int i = 0; i < n; i++) add(len[i]);
    }
    size_t add(int64_t len) {
        at.push_back(total);
        if (len <= limit) total += pad256((size_t)len);
        return at.back();
    }
    bool staged(int64_t len) const { return len > 0 && len <= limit; }  // the item has bytes in the buffer
};

// ---- a sub-stream of comp_len bytes at byte `pos` of a 256-byte-aligned buffer: the kernels get the address rounded down to
// 16 bytes, so that they keep their 16-byte loads wherever the stream lies, and the remainder as the offset of the first
// block; `skip` more bytes for a header that the host has read (2: zlib's)
struct SubStream {
    size_t base;       // from the buffer's first byte
    int32_t body_off;  // InfWrap::body_off
    int64_t in_len;    // from base to the stream's last byte
};
inline SubStream sub_stream(size_t pos, int64_t comp_len, int skip = 0) {
    return SubStream{pos & ~(size_t)15, (int32_t)(pos & 15) + skip, (int64_t)(pos & 15) + comp_len};
}

// ---- the two bytes of a zlib header (inflate.c HEAD): false with the code and the InfMsg of the first rule they break
inline bool zlib_head_check(const uint8_t *z, int64_t len, int *status, int *msg) {
    if (len < 2) *status = ZS_BUF_ERROR, *msg = kPartTruncated;
    else if ((z[0] & 15) != 8) *status = ZS_DATA_ERROR, *msg = kPartBadMethod;
    else if ((z[0] >> 4) > 7) *status = ZS_DATA_ERROR, *msg = kPartBadWindow;
    else if (((z[0] << 8) | z[1]) % 31) *status = ZS_DATA_ERROR, *msg = kPartBadHeaderCheck;
    else if (z[1] & 0x20) *status = ZS_NEED_DICT, *msg = kPartNeedDict;
    else return true;
    return false;
}

// ---- what becomes of one inflated sub-stream
// A stream that did not end fails with its own code and message, but one that ran out of output had more bytes than its
// container said: the room was that length, so the length is what is wrong.
inline void part_failure(int status, int msg, int *code, int *why) {
    const bool too_long = msg == kPartOutputFull;
    *code = too_long ? (int)ZS_DATA_ERROR : status, *why = too_long ? (int)kPartBadLength : msg;
}
enum PartLenRule { kLenAny, kLenExact, kLenAtLeast };  // the produced bytes against the container's length
enum PartClass { kPartDecoded, kPartFailed, kPartCallFailed };
struct PartVerdict {
    int cls;
    int code, msg;     // kPartFailed: the part's status and InfMsg
    bool trailer_cut;  // kPartDecoded: fewer than four bytes lie behind the last block (a zlib part ends inside its Adler-32)
};
// status / msg / out_len / used: what the inflate call gave for the stream (used: from the part's first byte); comp_len: the
// part's bytes in its file.  ZS_STREAM_ERROR or a status never written (ZS_OK): the call itself failed, its message stands.
inline PartVerdict part_verdict(int status, int msg, int64_t out_len, int64_t used, int64_t comp_len, PartLenRule rule, int64_t want) {
    PartVerdict v{kPartDecoded, ZS_OK, 0, false};
    if (status == ZS_STREAM_ERROR || status == ZS_OK) {
        v.cls = kPartCallFailed, v.code = ZS_STREAM_ERROR;
    } else if (status != ZS_STREAM_END) {
        v.cls = kPartFailed;
        part_failure(status, msg, &v.code, &v.msg);
    } else if ((rule == kLenExact && out_len != want) || (rule == kLenAtLeast && out_len < want)) {
        v.cls = kPartFailed, v.code = ZS_DATA_ERROR, v.msg = kPartBadLength;
    } else {
        v.trailer_cut = used + 4 > comp_len;
    }
    return v;
}

// ---- the codes of a call over files that have parts (entries, strips, tiles, chunks).  A part's reason is a string that
// outlives the call's end (a literal, a message table's entry); nothing is built per part unless it fails.
struct PartCodes {
    std::vector<int> &st;                        // per file: the caller's status vector
    std::vector<std::string> why;                // ... and why
    std::vector<std::vector<int>> pst;           // per file and part: ZS_OK or its code ...
    std::vector<std::vector<const char *>> pwhy;  // ... and why
    explicit PartCodes(std::vector<int> &file_status) : st(file_status), why(file_status.size()), pst(file_status.size()), pwhy(file_status.size()) {}
    void open_parts(int i, size_t count) { pst[(size_t)i].assign(count, ZS_OK), pwhy[(size_t)i].assign(count, ""); }
    void fail_file(int i, int code, const char *text) {  // (a file's first failure stays)
        if (st[(size_t)i] != ZS_OK) return;
        st[(size_t)i] = code, why[(size_t)i] = text;
    }
    void fail_part(int i, int64_t k, int code, const char *text) { pst[(size_t)i][(size_t)k] = code, pwhy[(size_t)i][(size_t)k] = text; }
    // the call's code and message: its first failing file's ("<file_noun> i: <why>"); *err stays where none failed
    int first_file(const char *file_noun, std::string *err) const {
        for (size_t i = 0; i < st.size(); i++)
            if (st[i] != ZS_OK) {
                char head[48];
                snprintf(head, sizeof head, "%s %lld: ", file_noun, (long long)i);
                *err = std::string(head) + why[i];
                return st[i];
            }
        return ZS_OK;
    }
    // A file's code is its first failing part's ("<part_noun> k: <why>"), the call's its first failing file's; *err is `before`
    // where none failed.  A file that was refused as a whole keeps its code, and its parts' codes are not copied out.
    int roll_up(const char *file_noun, const char *part_noun, int *const *part_status, const std::string &before, std::string *err) {
        for (size_t i = 0; i < st.size(); i++) {
            if (st[i] != ZS_OK) continue;
            if (part_status && part_status[i] && !pst[i].empty()) memcpy(part_status[i], pst[i].data(), sizeof(int) * pst[i].size());
            for (size_t k = 0; k < pst[i].size(); k++)
                if (pst[i][k] != ZS_OK) {
                    char head[48];
                    snprintf(head, sizeof head, "%s %lld: ", part_noun, (long long)k);
                    st[i] = pst[i][k], why[i] = std::string(head) + pwhy[i][k];
                    break;
                }
        }
        *err = before;
        return first_file(file_noun, err);
    }
};

// ---- the outputs of an encode call
// which fit: an output that is still ZS_OK and longer than its room gets ZS_BUF_ERROR, the first of them gives the call's code
// and text unless it has one; returns how many are ZS_OK
inline int mark_fit(std::vector<int> &st, const int64_t *out_len, const int64_t *out_cap, int *rc, std::string *err) {
    int n_fit = 0;
    for (size_t i = 0; i < st.size(); i++) {
        if (st[i] != ZS_OK) continue;
        if (out_cap[i] < out_len[i]) {
            st[i] = ZS_BUF_ERROR;
            if (*rc == ZS_OK) *rc = ZS_BUF_ERROR, *err = "buffer error";
        } else {
            n_fit++;
        }
    }
    return n_fit;
}
// a job over the fitting outputs failed: every output that is still ZS_OK takes its code
inline void fail_live(std::vector<int> &st, int code) {
    for (int &x : st)
        if (x == ZS_OK) x = code;
}

}  // namespace zs
