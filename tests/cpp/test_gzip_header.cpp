// The gzip header rules that the header kernel and the host's file walk share (zlibstream_amd/csrc/zs_gzip.h), run on the
// host over headers built here:
//   * every combination of FEXTRA / FNAME / FCOMMENT / FHCRC: the body offset, the name's place, MTIME / XFL / OS; every cut
//     of each of them is kGzTruncated -- or the header's own error where the cut leaves the deciding bytes in --, the whole
//     header with nothing behind it is accepted;
//   * both sides of every error class: the magic's two bytes, CM 8 against 7 and 9, each reserved flag bit against each
//     legal one, FHCRC right against each of its 16 bits flipped and against a header byte changed under it;
//   * FEXTRA: XLEN 0, a BGZF subfield alone, one behind another subfield, a BGZF-like subfield with SLEN != 2 (not BGZF),
//     a subfield list that does not add up to XLEN (not an error: nobody has to read it);
//   * a name of 0, 1 and 300 bytes, and a name with no terminator;
//   * the ten bytes the encoder writes read back, XFL by level.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_gzip.h"

using namespace zs;

static int fails = 0, checks = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        checks++;                             \
        if (!(cond)) {                        \
            if (fails++ < 20) {               \
                printf("FAIL %s: ", #cond);   \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

typedef std::vector<uint8_t> Bytes;

static uint32_t crc_bitwise(const uint8_t *p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

struct Spec {
    int flg = 0;
    Bytes extra;  // FEXTRA's bytes (without XLEN)
    std::string name, comment;
    uint32_t mtime = 0x01020304;
    int xfl = 2, os = 3;
};
static Bytes subfield(int si1, int si2, const Bytes &data) {
    Bytes b = {(uint8_t)si1, (uint8_t)si2, (uint8_t)(data.size() & 255), (uint8_t)(data.size() >> 8)};
    b.insert(b.end(), data.begin(), data.end());
    return b;
}
static Bytes build(const Spec &s) {
    Bytes h = {0x1F, 0x8B, 8, (uint8_t)s.flg, (uint8_t)s.mtime, (uint8_t)(s.mtime >> 8), (uint8_t)(s.mtime >> 16), (uint8_t)(s.mtime >> 24),
               (uint8_t)s.xfl, (uint8_t)s.os};
    if (s.flg & 4) {
        h.push_back((uint8_t)(s.extra.size() & 255)), h.push_back((uint8_t)(s.extra.size() >> 8));
        h.insert(h.end(), s.extra.begin(), s.extra.end());
    }
    if (s.flg & 8) h.insert(h.end(), s.name.begin(), s.name.end()), h.push_back(0);
    if (s.flg & 16) h.insert(h.end(), s.comment.begin(), s.comment.end()), h.push_back(0);
    if (s.flg & 2) {
        const uint32_t c = crc_bitwise(h.data(), h.size());
        h.push_back((uint8_t)c), h.push_back((uint8_t)(c >> 8));
    }
    return h;
}
static int parse(const Bytes &b, size_t len, GzHeader *h) {
    // exactly `len` bytes in a buffer of their own: a read past them is a sanitizer build's to see
    Bytes exact(b.begin(), b.begin() + (long)len);
    return gzip_parse_header(exact.data(), (int64_t)exact.size(), h);
}

int main() {
    GzHeader h;
    // ---- every FLG combination, whole, cut at every byte, and with a body behind it
    size_t longest = 0;
    for (int bits = 0; bits < 16; bits++) {
        Spec s;
        s.flg = (bits & 1 ? 4 : 0) | (bits & 2 ? 8 : 0) | (bits & 4 ? 16 : 0) | (bits & 8 ? 2 : 0);
        s.extra = subfield('A', 'p', {1, 2, 3});
        s.name = "file.txt", s.comment = "a comment";
        const Bytes b = build(s);
        longest = b.size() > longest ? b.size() : longest;
        CHECK(parse(b, b.size(), &h) == kGzOk, "flg %d", s.flg);
        CHECK(h.body_off == (int64_t)b.size(), "flg %d: body at %lld of %zu", s.flg, (long long)h.body_off, b.size());
        CHECK(h.mtime == s.mtime && h.xfl == 2 && h.os == 3 && h.flg == s.flg && h.member_size == 0, "flg %d: fields", s.flg);
        if (s.flg & 8) CHECK(h.name_len == 8 && memcmp(b.data() + h.name_off, "file.txt", 8) == 0, "flg %d: name", s.flg);
        else CHECK(h.name_off == 0 && h.name_len == 0, "flg %d: no name", s.flg);
        for (size_t cut = 0; cut < b.size(); cut++) CHECK(parse(b, cut, &h) == kGzTruncated, "flg %d cut at %zu of %zu", s.flg, cut, b.size());
        Bytes more = b;
        more.insert(more.end(), {0x03, 0x00, 9, 9, 9});
        CHECK(parse(more, more.size(), &h) == kGzOk && h.body_off == (int64_t)b.size(), "flg %d with a body", s.flg);
    }
    CHECK(longest == 10 + 2 + 7 + 9 + 10 + 2, "the full header is %zu bytes", longest);
    // ---- the error classes, both sides
    {
        Spec s;
        const Bytes ok = build(s);
        CHECK(parse(ok, ok.size(), &h) == kGzOk && h.body_off == 10, "plain header");
        for (int k = 0; k < 2; k++)
            for (int bit = 0; bit < 8; bit++) {
                Bytes b = ok;
                b[(size_t)k] ^= (uint8_t)(1 << bit);
                CHECK(parse(b, b.size(), &h) == kGzBadMagic, "magic byte %d bit %d", k, bit);
                CHECK(parse(b, 2, &h) == kGzBadMagic && parse(b, 1, &h) == kGzTruncated, "magic alone, byte %d bit %d", k, bit);
            }
        for (int cm : {0, 7, 9, 255}) {
            Bytes b = ok;
            b[2] = (uint8_t)cm;
            CHECK(parse(b, b.size(), &h) == kGzBadMethod, "CM %d", cm);
            CHECK(parse(b, 4, &h) == kGzBadMethod && parse(b, 3, &h) == kGzTruncated, "CM %d in four bytes", cm);
        }
        for (int bit = 0; bit < 8; bit++) {
            Spec t;
            t.flg = 1 << bit;  // (FTEXT, bit 0, says nothing about the layout)
            t.extra = {}, t.name = "n", t.comment = "c";
            const Bytes b = build(t);
            const int want = bit >= 5 ? (int)kGzBadFlags : (int)kGzOk;
            CHECK(parse(b, b.size(), &h) == want, "flag bit %d gives %d", bit, parse(b, b.size(), &h));
        }
        Bytes b = ok;
        b[3] = 0xE0 | 0x1F;
        CHECK(parse(b, b.size(), &h) == kGzBadFlags, "all flags");
        b[2] = 7;
        CHECK(parse(b, b.size(), &h) == kGzBadMethod, "the method is judged in front of the flags");
    }
    {
        Spec s;
        s.flg = 2 | 8 | 4;
        s.extra = subfield('x', 'y', {7});
        s.name = "crc";
        const Bytes ok = build(s);
        CHECK(parse(ok, ok.size(), &h) == kGzOk, "FHCRC right");
        for (int bit = 0; bit < 16; bit++) {
            Bytes b = ok;
            b[b.size() - 2 + (size_t)(bit >> 3)] ^= (uint8_t)(1 << (bit & 7));
            CHECK(parse(b, b.size(), &h) == kGzBadHcrc, "FHCRC bit %d", bit);
        }
        for (size_t at = 4; at + 2 < ok.size(); at++) {  // a header byte under the CRC (not one that moves the layout)
            if (at == 10 || at == 11 || at == 14 || at == 15 || ok[at] == 0) continue;
            Bytes b = ok;
            b[at] ^= 0x40;
            CHECK(parse(b, b.size(), &h) == kGzBadHcrc, "header byte %zu changed under FHCRC", at);
        }
    }
    // ---- FEXTRA
    {
        Spec s;
        s.flg = 4;
        Bytes b = build(s);  // XLEN 0
        CHECK(b.size() == 12 && parse(b, b.size(), &h) == kGzOk && h.body_off == 12 && h.member_size == 0, "XLEN 0");
        s.extra = subfield(66, 67, {0x33, 0x12});
        b = build(s);
        CHECK(parse(b, b.size(), &h) == kGzOk && h.body_off == 18 && h.member_size == 0x1233 + 1, "BGZF alone: %lld", (long long)h.member_size);
        s.extra = subfield('R', 'A', {1, 2, 3, 4, 5});
        const Bytes bc = subfield(66, 67, {0xFF, 0xFF});
        s.extra.insert(s.extra.end(), bc.begin(), bc.end());
        b = build(s);
        CHECK(parse(b, b.size(), &h) == kGzOk && h.body_off == 12 + 9 + 6 && h.member_size == 65536, "BGZF behind another subfield: %lld", (long long)h.member_size);
        s.extra = subfield(66, 67, {1, 2, 3});
        b = build(s);
        CHECK(parse(b, b.size(), &h) == kGzOk && h.member_size == 0, "SLEN 3 is not BGZF");
        s.extra = subfield(66, 67, {1});
        b = build(s);
        CHECK(parse(b, b.size(), &h) == kGzOk && h.member_size == 0, "SLEN 1 is not BGZF");
        s.extra = subfield(66, 68, {1, 2});
        b = build(s);
        CHECK(parse(b, b.size(), &h) == kGzOk && h.member_size == 0, "SI2 68 is not BGZF");
        s.extra = {66, 67, 9, 0, 1, 2};  // SLEN says 9, XLEN holds 2 more bytes
        b = build(s);
        CHECK(parse(b, b.size(), &h) == kGzOk && h.member_size == 0 && h.body_off == 18, "a subfield that overruns XLEN");
        s.extra = {66, 67, 2};  // three bytes: no room for a subfield's head
        b = build(s);
        CHECK(parse(b, b.size(), &h) == kGzOk && h.member_size == 0 && h.body_off == 15, "XLEN 3");
    }
    // ---- names
    for (size_t len : {(size_t)0, (size_t)1, (size_t)300}) {
        Spec s;
        s.flg = 8;
        s.name = std::string(len, 'n');
        const Bytes b = build(s);
        CHECK(parse(b, b.size(), &h) == kGzOk && h.name_off == 10 && h.name_len == (int64_t)len && h.body_off == (int64_t)(11 + len), "a name of %zu bytes", len);
        Bytes open_end(b.begin(), b.end() - 1);  // no terminator: the name runs to the end of the input
        CHECK(parse(open_end, open_end.size(), &h) == kGzTruncated, "a name of %zu bytes with no terminator", len);
        open_end.insert(open_end.end(), 500, 'x');
        CHECK(parse(open_end, open_end.size(), &h) == kGzTruncated, "... and 500 more bytes of it");
    }
    // ---- what the encoder writes
    for (int level = -1; level <= 9; level++) {
        uint8_t hd[kGzipHeadBytes];
        gzip_put_header(hd, level);
        CHECK(gzip_parse_header(hd, kGzipHeadBytes, &h) == kGzOk && h.body_off == 10 && h.mtime == 0 && h.os == 255 && h.flg == 0, "level %d", level);
        CHECK(h.xfl == (level == 9 ? 2 : level == 1 ? 4 : 0), "XFL %d at level %d", h.xfl, level);
    }
    CHECK(wrap_head_bytes(kWrapZlib) == 2 && wrap_tail_bytes(kWrapZlib) == 4 && wrap_head_bytes(kWrapRaw) == 0 && wrap_tail_bytes(kWrapRaw) == 0 &&
              wrap_head_bytes(kWrapGzip) == 10 && wrap_tail_bytes(kWrapGzip) == 8,
          "the containers' sizes");
    if (fails) {
        printf("%d of %d checks failed\n", fails, checks);
        return 1;
    }
    printf("PASS %d checks\n", checks);
    return 0;
}
