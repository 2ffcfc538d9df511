// zs_gzip.h -- the gzip member header (RFC 1952), the rules that the header kernel (zs_inflate_par.hip, zs_gzip_header_kernel),
// the host's walk over a file's members (zs_wrap_host.inc) and tests/cpp/test_gzip_header.cpp share; and the framing constants
// of the three containers the batch calls read and write (include/zsgpu.h ZS_WRAP_*).
//
// A member:  1f 8b | CM = 8 | FLG | MTIME (4, little-endian) | XFL | OS | [XLEN (2) and XLEN bytes of subfields]   FEXTRA  0x04
//            | [name, zero-terminated]  FNAME 0x08 | [comment, zero-terminated]  FCOMMENT 0x10 | [CRC16]  FHCRC 0x02
//            | deflate body | CRC-32 (4) | ISIZE (4, input length mod 2^32)
// CRC16 is the low 16 bits of the CRC-32 of every header byte in front of it.  A subfield is SI1, SI2, SLEN (2), SLEN bytes;
// BGZF (the SAM/BAM specification, section 4.1) marks its members with SI1 = 66, SI2 = 67, SLEN = 2 and the member's total
// size minus one in those two bytes.
#pragma once

#include <cstdint>

#include "zs_crc32.h"

namespace zs {

enum { kWrapZlib = 0, kWrapRaw = 1, kWrapGzip = 2 };
constexpr int kGzipHeadBytes = 10, kGzipTrailBytes = 8;

// what is wrong with a header, in zlib's classes (inflate.c: HEAD .. HCRC): the host turns these into its messages
enum GzErr { kGzOk = 0, kGzTruncated, kGzBadMagic, kGzBadMethod, kGzBadFlags, kGzBadHcrc };

struct GzHeader {
    int64_t body_off;     // where the deflate body begins
    int64_t member_size;  // BGZF: the whole member, header to ISIZE (BSIZE + 1); 0: no BGZF subfield
    int64_t name_off, name_len;  // FNAME without its terminator; name_off 0: the member has none
    uint32_t mtime;
    int32_t xfl, os, flg;
};

// Reads the header of the member at p[0 .. len).  kGzOk and *h, or the first thing wrong in the order zlib finds it; bytes
// that are not there are kGzTruncated wherever the header ends in them (also inside a name that has no terminator).
ZS_HD int gzip_parse_header(const uint8_t *p, int64_t len, GzHeader *h) {
    h->body_off = 0, h->member_size = 0, h->name_off = 0, h->name_len = 0, h->mtime = 0, h->xfl = 0, h->os = 0, h->flg = 0;
    if (len < 2) return kGzTruncated;
    if (p[0] != 0x1F || p[1] != 0x8B) return kGzBadMagic;
    if (len < 4) return kGzTruncated;
    if (p[2] != 8) return kGzBadMethod;
    const int flg = p[3];
    if (flg & 0xE0) return kGzBadFlags;
    if (len < kGzipHeadBytes) return kGzTruncated;
    h->flg = flg;
    h->mtime = (uint32_t)p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24;
    h->xfl = p[8], h->os = p[9];
    int64_t at = kGzipHeadBytes;
    if (flg & 0x04) {
        if (at + 2 > len) return kGzTruncated;
        const int64_t xlen = (int64_t)p[at] | (int64_t)p[at + 1] << 8;
        at += 2;
        if (at + xlen > len) return kGzTruncated;
        // the subfields: a list that does not add up to XLEN is no error of the member (zlib does not read it at all), the
        // walk ends where the next subfield would not fit
        for (int64_t s = at; s + 4 <= at + xlen;) {
            const int64_t slen = (int64_t)p[s + 2] | (int64_t)p[s + 3] << 8;
            if (s + 4 + slen > at + xlen) break;
            if (p[s] == 66 && p[s + 1] == 67 && slen == 2 && h->member_size == 0) h->member_size = ((int64_t)p[s + 4] | (int64_t)p[s + 5] << 8) + 1;
            s += 4 + slen;
        }
        at += xlen;
    }
    if (flg & 0x08) {
        const int64_t a0 = at;
        while (at < len && p[at] != 0) at++;
        if (at >= len) return kGzTruncated;
        h->name_off = a0, h->name_len = at - a0;
        at++;
    }
    if (flg & 0x10) {
        while (at < len && p[at] != 0) at++;
        if (at >= len) return kGzTruncated;
        at++;
    }
    if (flg & 0x02) {
        if (at + 2 > len) return kGzTruncated;
        // (bit-serial: a header is a few dozen bytes, and most members carry no FHCRC)
        const uint32_t crc = crc32_bytes_slow(0, p, (uint64_t)at);
        if ((crc & 0xFFFFu) != ((uint32_t)p[at] | (uint32_t)p[at + 1] << 8)) return kGzBadHcrc;
        at += 2;
    }
    h->body_off = at;
    return kGzOk;
}

// XFL of a member this library writes: what zlib's deflate puts there, 2 for its best level, 4 for its fastest
ZS_HD int gzip_xfl(int level) { return level == 9 ? 2 : level == 1 ? 4 : 0; }
// the ten header bytes: no flags, MTIME 0, OS 255 (unknown)
ZS_HD void gzip_put_header(uint8_t *p, int level) {
    p[0] = 0x1F, p[1] = 0x8B, p[2] = 8, p[3] = 0, p[4] = 0, p[5] = 0, p[6] = 0, p[7] = 0, p[8] = (uint8_t)gzip_xfl(level), p[9] = 255;
}
// bytes a container adds to the deflate body; the zlib stream the engine writes has 2 in front and 4 behind
ZS_HD int wrap_head_bytes(int wrap) { return wrap == kWrapGzip ? kGzipHeadBytes : wrap == kWrapZlib ? 2 : 0; }
ZS_HD int wrap_tail_bytes(int wrap) { return wrap == kWrapGzip ? kGzipTrailBytes : wrap == kWrapZlib ? 4 : 0; }

}  // namespace zs
