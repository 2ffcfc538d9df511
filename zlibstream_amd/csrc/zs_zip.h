// zs_zip.h -- the ZIP container (PKWARE APPNOTE 6.3, sections 4.3 and 4.5.3): the rules by which the host finds an archive's
// end record, walks its central directory and places every entry's body (zs_zip_host.inc, zs_zip_file_info and
// zs_zip_decode_files_batch), the bytes the writer puts around the bodies (zs_zip_encode_batch_device) and the descriptor
// of the closing kernel (zs_zip.hip); tests/cpp/test_zip_walk.cpp runs them on the host.  Nothing here reads outside
// [file, file + len).
//
// An archive:  per entry [local header (30) | name | extra | body | optional data descriptor]
//              central directory: per entry [record (46) | name | extra | comment]
//              [ZIP64 end record (56 ..) | ZIP64 locator (20)]  end record (22) | comment
// All numbers little-endian.  A reader goes by the central directory alone: the local header gives only the place of the
// body (its own name and extra lengths), and where flag bit 3 is set its CRC and sizes are zero -- they follow the body in a
// data descriptor that nobody needs who has the directory.
// The ZIP64 forms: a 16- or 32-bit field that is all ones stands for a value in the ZIP64 end record (end record fields) or in
// the extra field with header id 0x0001 (central record fields; in the order size, compressed size, local offset, and only
// those that are all ones).
// Bytes in front of the first local header (a self-extractor) move everything behind them: the offsets of such an archive
// are short by `shift`, which is what the place of the end record and the directory's own length and offset leave over.
#pragma once

#include <cstdint>

#include "zs_crc32.h"

namespace zs {

constexpr int kZipLocalBytes = 30, kZipCentralBytes = 46, kZipEndBytes = 22, kZipEnd64Bytes = 56, kZipLocatorBytes = 20;
constexpr uint32_t kZipSigLocal = 0x04034B50u, kZipSigCentral = 0x02014B50u, kZipSigEnd = 0x06054B50u, kZipSigEnd64 = 0x06064B50u,
                   kZipSigLocator = 0x07064B50u;
constexpr int kZipStored = 0, kZipDeflated = 8, kZipAuto = -1;
constexpr int64_t kZipMaxLen = 0x7FFFFFFF - 1024;  // an entry, a file and a file's output, in one call of the engine

// what is wrong: with the file (its walk ends) or with one entry (the walk goes on)
enum ZipErr {
    kZipOk = 0,
    kZipNoEnd, kZipShortFile, kZipMultiDisk, kZipBadEnd64, kZipBadShift, kZipBadDirectory,  // the file
    kZipEncrypted, kZipBadMethod, kZipStoredLength, kZipLocalMismatch, kZipTruncated        // an entry
};
// the library's codes (include/zsgpu.h ZS_DATA_ERROR, ZS_BUF_ERROR) and messages of these
ZS_HD int zip_err_status(int e) { return e == kZipOk ? 0 : (e == kZipShortFile || e == kZipTruncated) ? -5 : -3; }
inline const char *zip_err_message(int e) {
    switch (e) {
    case kZipOk: return "";
    case kZipNoEnd: return "end of central directory record not found";
    case kZipMultiDisk: return "multi-disk archives are not supported";
    case kZipBadEnd64: return "invalid ZIP64 end of central directory record";
    case kZipBadShift: return "central directory overlaps the end record";
    case kZipBadDirectory: return "invalid central directory";
    case kZipEncrypted: return "encrypted entries are not supported";
    case kZipBadMethod: return "unsupported compression method";
    case kZipStoredLength: return "incorrect length check";
    case kZipLocalMismatch: return "local header mismatch";
    default: return "buffer error";
    }
}

// the two structs of include/zsgpu.h (zs_zip_info, zs_zip_entry), field for field
struct ZipInfo {
    int64_t n_entries, total_len;
    int64_t cd_off, cd_len, shift;
    int64_t comment_off, comment_len;
    int zip64;
};
struct ZipEntry {
    int64_t name_off;
    int name_len;
    int method, flags;
    uint32_t crc32;
    int64_t comp_len, len, local_off, body_off, out_off;
    uint16_t dos_time, dos_date;
    uint32_t external_attr;
    int status;
};

ZS_HD uint32_t zip_le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
ZS_HD uint32_t zip_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
ZS_HD uint64_t zip_le64(const uint8_t *p) { return (uint64_t)zip_le32(p) | (uint64_t)zip_le32(p + 4) << 32; }
ZS_HD void zip_put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8); }
ZS_HD void zip_put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24); }
// a 64-bit field no file this library is given can mean (it would not fit an int64_t's sums either)
constexpr uint64_t kZipHuge = (uint64_t)1 << 62;

// The end record, and the ZIP64 one where the file has it: *info without total_len, the directory's place with the shift
// applied.  The search goes backwards over the last 22 + 65535 bytes and takes the first signature whose comment length
// reaches exactly the end of the file, so a comment that holds the signature does not win over the record it belongs to.
ZS_HD int zip_find_end(const uint8_t *f, int64_t len, ZipInfo *info) {
    info->n_entries = 0, info->total_len = 0, info->cd_off = 0, info->cd_len = 0, info->shift = 0, info->comment_off = 0, info->comment_len = 0, info->zip64 = 0;
    if (len < kZipEndBytes) return kZipShortFile;
    const int64_t last = len - kZipEndBytes, first = last > 65535 ? last - 65535 : 0;
    int64_t pos = -1;
    for (int64_t p = last; p >= first; p--)
        if (f[p] == 0x50 && zip_le32(f + p) == kZipSigEnd && p + kZipEndBytes + (int64_t)zip_le16(f + p + 20) == len) {
            pos = p;
            break;
        }
    if (pos < 0) return kZipNoEnd;
    const uint8_t *e = f + pos;
    uint64_t disk = zip_le16(e + 4), cd_disk = zip_le16(e + 6), n_here = zip_le16(e + 8), n_all = zip_le16(e + 10), cd_len = zip_le32(e + 12), cd_off = zip_le32(e + 16);
    info->comment_off = pos + kZipEndBytes, info->comment_len = (int64_t)zip_le16(e + 20);
    int64_t end_pos = pos;  // where the directory ends if nothing lies in front of the archive
    const bool saturated = disk == 0xFFFF || cd_disk == 0xFFFF || n_here == 0xFFFF || n_all == 0xFFFF || cd_len == 0xFFFFFFFFu || cd_off == 0xFFFFFFFFu;
    if (pos >= kZipLocatorBytes && zip_le32(f + pos - kZipLocatorBytes) == kZipSigLocator) {
        const uint8_t *l = f + pos - kZipLocatorBytes;
        // the record stands in front of its locator (also in a prefixed archive, where the locator's offset is short by the
        // shift); one with an extensible data sector is longer and is found by the offset
        int64_t rec = pos - kZipLocatorBytes - kZipEnd64Bytes;
        if (rec < 0 || zip_le32(f + rec) != kZipSigEnd64) {
            const uint64_t by_off = zip_le64(l + 8);
            rec = by_off <= (uint64_t)(pos - kZipLocatorBytes) && (int64_t)by_off + kZipEnd64Bytes <= pos - kZipLocatorBytes && zip_le32(f + by_off) == kZipSigEnd64 ? (int64_t)by_off : -1;
        }
        if (rec >= 0) {
            if (zip_le32(l + 4) != 0 || zip_le32(l + 16) > 1) return kZipMultiDisk;
            const uint8_t *r = f + rec;
            if (zip_le64(r + 4) < (uint64_t)kZipEnd64Bytes - 12) return kZipBadEnd64;
            if (disk == 0xFFFF) disk = zip_le32(r + 16);
            if (cd_disk == 0xFFFF) cd_disk = zip_le32(r + 20);
            if (n_here == 0xFFFF) n_here = zip_le64(r + 24);
            if (n_all == 0xFFFF) n_all = zip_le64(r + 32);
            if (cd_len == 0xFFFFFFFFu) cd_len = zip_le64(r + 40);
            if (cd_off == 0xFFFFFFFFu) cd_off = zip_le64(r + 48);
            info->zip64 = 1, end_pos = rec;
        } else if (saturated) {
            return kZipBadEnd64;
        }
    }
    // (an end record with all-ones fields and no ZIP64 record means what it says: 65535 entries, and so on)
    if (disk != 0 || cd_disk != 0 || n_here != n_all) return kZipMultiDisk;
    if (n_all >= kZipHuge || cd_len >= kZipHuge || cd_off >= kZipHuge) return kZipBadDirectory;
    if ((int64_t)cd_len > end_pos || (int64_t)cd_off > end_pos - (int64_t)cd_len) return kZipBadShift;
    info->shift = end_pos - (int64_t)cd_len - (int64_t)cd_off;
    info->cd_off = (int64_t)cd_off + info->shift, info->cd_len = (int64_t)cd_len, info->n_entries = (int64_t)n_all;
    if (n_all > cd_len / kZipCentralBytes) return kZipBadDirectory;  // (more records than the directory has room for)
    return kZipOk;
}

// The central record at *at of the directory that ends at `end`: *e without out_off, body_off and status, *at behind the
// record.  kZipBadDirectory for a record that is not one or does not lie inside the directory.
ZS_HD int zip_read_record(const uint8_t *f, int64_t end, int64_t shift, int64_t *at, ZipEntry *e) {
    const int64_t a = *at;
    if (end - a < kZipCentralBytes || zip_le32(f + a) != kZipSigCentral) return kZipBadDirectory;
    const uint8_t *r = f + a;
    const int64_t n_name = zip_le16(r + 28), n_extra = zip_le16(r + 30), n_comment = zip_le16(r + 32);
    if (end - a - kZipCentralBytes < n_name + n_extra + n_comment) return kZipBadDirectory;
    e->flags = (int)zip_le16(r + 8), e->method = (int)zip_le16(r + 10);
    e->dos_time = (uint16_t)zip_le16(r + 12), e->dos_date = (uint16_t)zip_le16(r + 14);
    e->crc32 = zip_le32(r + 16);
    uint64_t comp = zip_le32(r + 20), size = zip_le32(r + 24), off = zip_le32(r + 42);
    e->external_attr = zip_le32(r + 38);
    e->name_off = a + kZipCentralBytes, e->name_len = (int)n_name;
    if (comp == 0xFFFFFFFFu || size == 0xFFFFFFFFu || off == 0xFFFFFFFFu) {
        // the ZIP64 extra field: eight bytes for each of the three that is all ones, in this order
        const uint8_t *x = r + kZipCentralBytes + n_name;
        for (int64_t s = 0; s + 4 <= n_extra;) {
            const int64_t id = zip_le16(x + s), sz = zip_le16(x + s + 2);
            if (s + 4 + sz > n_extra) break;
            if (id == 0x0001) {
                int64_t q = s + 4;
                const int64_t q_end = q + sz;
                uint64_t *const want[3] = {&size, &comp, &off};
                for (int k = 0; k < 3; k++)
                    if (*want[k] == 0xFFFFFFFFu) {
                        if (q + 8 > q_end) return kZipBadDirectory;
                        *want[k] = zip_le64(x + q), q += 8;
                    }
                break;
            }
            s += 4 + sz;
        }
        // (without the field the values stand as they are: four gigabytes less one is a length like another)
    }
    if (comp >= kZipHuge || size >= kZipHuge || off >= kZipHuge) return kZipBadDirectory;
    e->comp_len = (int64_t)comp, e->len = (int64_t)size, e->local_off = (int64_t)off + shift;
    e->body_off = 0, e->out_off = 0, e->status = 0;
    *at = a + kZipCentralBytes + n_name + n_extra + n_comment;
    return kZipOk;
}

// What keeps the engine from decoding entry *e of the file, in the order a reader meets it; sets body_off.
ZS_HD int zip_check_entry(const uint8_t *f, int64_t len, ZipEntry *e) {
    if (e->flags & (1 | 1 << 6 | 1 << 13)) return kZipEncrypted;
    if (e->method != kZipStored && e->method != kZipDeflated) return kZipBadMethod;
    if (e->method == kZipStored && e->comp_len != e->len) return kZipStoredLength;
    const int64_t lo = e->local_off;
    if (lo > len - 4) return kZipTruncated;
    if (zip_le32(f + lo) != kZipSigLocal) return kZipLocalMismatch;
    if (lo > len - kZipLocalBytes) return kZipTruncated;
    const int64_t n_name = zip_le16(f + lo + 26), n_extra = zip_le16(f + lo + 28);
    if (n_name != e->name_len) return kZipLocalMismatch;
    if (len - lo - kZipLocalBytes < n_name) return kZipTruncated;
    for (int64_t k = 0; k < n_name; k++)
        if (f[lo + kZipLocalBytes + k] != f[e->name_off + k]) return kZipLocalMismatch;
    if (len - lo - kZipLocalBytes - n_name < n_extra) return kZipTruncated;
    e->body_off = lo + kZipLocalBytes + n_name + n_extra;
    if (e->comp_len > len - e->body_off) return kZipTruncated;
    return kZipOk;
}

// The whole walk.  kZipOk and *info (total_len included); the first `cap` entries in entries[] (may be null with cap 0), each
// with status 0 or the library's code for what zip_check_entry found, which errs[] (may be null) names.  Otherwise the file's
// error, with *info as far as zip_find_end got.
inline int zip_walk(const uint8_t *f, int64_t len, ZipInfo *info, ZipEntry *entries, int64_t cap, uint8_t *errs) {
    const int rc = zip_find_end(f, len, info);
    if (rc != kZipOk) return rc;
    const int64_t end = info->cd_off + info->cd_len;
    int64_t at = info->cd_off, total = 0;
    for (int64_t i = 0; i < info->n_entries; i++) {
        ZipEntry e;
        const int rr = zip_read_record(f, end, info->shift, &at, &e);
        if (rr != kZipOk) return rr;
        const int why = zip_check_entry(f, len, &e);
        e.status = zip_err_status(why), e.out_off = total;
        total = total > INT64_MAX - e.len ? INT64_MAX : total + e.len;
        if (i < cap) {
            entries[i] = e;
            if (errs) errs[i] = (uint8_t)why;
        }
    }
    if (at != end) return kZipBadDirectory;  // records behind the last one the end record counts
    info->total_len = total;
    return kZipOk;
}

// ---- the writer: version needed 2.0 for a deflated entry, 1.0 for a stored one, no extra field, no data descriptor, no
// comments; the CRC fields are left zero (the closing kernel fills them, zs_zip.hip)
ZS_HD uint32_t zip_version_needed(int method) { return method == kZipDeflated ? 20 : 10; }
ZS_HD void zip_put_local(uint8_t *p, int method, int utf8, uint32_t dos_time, uint32_t dos_date, uint32_t comp_len, uint32_t len, uint32_t name_len) {
    zip_put32(p, kZipSigLocal), zip_put16(p + 4, zip_version_needed(method)), zip_put16(p + 6, utf8 ? 1u << 11 : 0), zip_put16(p + 8, (uint32_t)method);
    zip_put16(p + 10, dos_time), zip_put16(p + 12, dos_date), zip_put32(p + 14, 0), zip_put32(p + 18, comp_len), zip_put32(p + 22, len);
    zip_put16(p + 26, name_len), zip_put16(p + 28, 0);
}
// "version made by": 2.0, and the host byte 3 (Unix) when the attributes carry a Unix mode in their high half, else 0
ZS_HD void zip_put_central(uint8_t *p, int method, int utf8, uint32_t dos_time, uint32_t dos_date, uint32_t comp_len, uint32_t len, uint32_t name_len,
                           uint32_t external_attr, uint32_t local_off) {
    zip_put32(p, kZipSigCentral), zip_put16(p + 4, ((external_attr >> 16) ? 3u << 8 : 0) | 20), zip_put16(p + 6, zip_version_needed(method));
    zip_put16(p + 8, utf8 ? 1u << 11 : 0), zip_put16(p + 10, (uint32_t)method), zip_put16(p + 12, dos_time), zip_put16(p + 14, dos_date);
    zip_put32(p + 16, 0), zip_put32(p + 20, comp_len), zip_put32(p + 24, len), zip_put16(p + 28, name_len), zip_put16(p + 30, 0), zip_put16(p + 32, 0);
    zip_put16(p + 34, 0), zip_put16(p + 36, 0), zip_put32(p + 38, external_attr), zip_put32(p + 42, local_off);
}
ZS_HD void zip_put_eocd(uint8_t *p, uint32_t n_entries, uint32_t cd_len, uint32_t cd_off) {
    zip_put32(p, kZipSigEnd), zip_put16(p + 4, 0), zip_put16(p + 6, 0), zip_put16(p + 8, n_entries), zip_put16(p + 10, n_entries);
    zip_put32(p + 12, cd_len), zip_put32(p + 16, cd_off), zip_put16(p + 20, 0);
}

// Room for one entry's body: an entry the caller forces to be deflated can grow to the raw stream's bound (the engine's
// zlib bound less the six bytes of that container, `deflate_bound`); under kZipAuto the stored form is kept unless the
// deflated one is shorter, so neither that nor a stored entry is ever longer than its data.
ZS_HD int64_t zip_body_bound(int64_t len, int method, int64_t deflate_bound) { return method == kZipDeflated && len > 0 ? deflate_bound - 6 : len; }
// an entry's share of the archive (local header, name, body, central record, name), and the archive around the shares
ZS_HD int64_t zip_entry_bound(int64_t body_bound, int name_len) { return kZipLocalBytes + kZipCentralBytes + 2 * (int64_t)name_len + body_bound; }
ZS_HD int64_t zip_bound(int64_t entry_bounds) { return entry_bounds + kZipEndBytes; }

// ---- the closing kernel's descriptor (KZ, zs_zip.hip): where entry's CRC-32 goes, and which span of the KC job computed it
struct ZipClose {
    uint8_t *local_crc, *central_crc;  // local header + 14, central record + 16: any alignment
    uint32_t span, pad;
};

}  // namespace zs
