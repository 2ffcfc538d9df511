// The ZIP rules that the engine's host side runs (zlibstream_amd/csrc/zs_zip.h), on the host, built with
// -fsanitize=address,undefined by tests/test_zip_host.py and given only heap blocks of exactly the bytes it may read:
//   * every file named on the command line (archives written by Python's zipfile: plain, force_zip64, data descriptors) and
//     the archives built here, whole and cut at every byte: the whole one walks, no proper prefix does, nothing is read past
//     the end of any;
//   * both sides of every rule: the legal archive built here, and the same bytes with one field changed --
//     the end record (a signature inside the comment, disk numbers, counts), the ZIP64 end record and locator, the ZIP64
//     extra field and its order, bytes in front of the archive and a directory that would begin in front of the file,
//     the directory's signatures, lengths, end and count, and per entry the flag bits, the method, a stored entry's lengths,
//     the local header's signature, name length, name bytes and extra field, a body that reaches past the file;
//   * the writer's records read back by the reader, and the bound.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_zip.h"

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
static void put16(Bytes &b, uint32_t v) { b.push_back((uint8_t)v), b.push_back((uint8_t)(v >> 8)); }
static void put32(Bytes &b, uint32_t v) { put16(b, v & 0xFFFF), put16(b, v >> 16); }
static void put64(Bytes &b, uint64_t v) { put32(b, (uint32_t)v), put32(b, (uint32_t)(v >> 32)); }
static void puts_(Bytes &b, const std::string &s) { b.insert(b.end(), s.begin(), s.end()); }
static void poke16(Bytes &b, size_t at, uint32_t v) { b[at] = (uint8_t)v, b[at + 1] = (uint8_t)(v >> 8); }
static void poke32(Bytes &b, size_t at, uint32_t v) { poke16(b, at, v & 0xFFFF), poke16(b, at + 2, v >> 16); }

struct Ent {
    std::string name;
    int method;
    uint32_t size;  // (the walk decodes nothing: a deflated entry's body is any bytes)
    Bytes body, local_extra, central_extra;
    int flags = 0;
    // ZIP64 in the central record: which of size / comp / offset are written all ones (bits 0, 1, 2)
    int saturate = 0;
};
struct Places {
    std::vector<size_t> local, body, record;
    size_t cd_off = 0, cd_len = 0, end64 = 0, end = 0;
};
struct Opt {
    std::string prefix, comment;
    bool end64 = false;
};

static Bytes build(const std::vector<Ent> &ents, const Opt &o, Places *pl) {
    Bytes b;
    *pl = Places();
    for (const Ent &e : ents) {
        pl->local.push_back(b.size());
        put32(b, kZipSigLocal), put16(b, 20), put16(b, (uint32_t)e.flags), put16(b, (uint32_t)e.method), put16(b, 0), put16(b, 0x21);
        put32(b, 0x11223344u), put32(b, (uint32_t)e.body.size()), put32(b, e.size), put16(b, (uint32_t)e.name.size()), put16(b, (uint32_t)e.local_extra.size());
        puts_(b, e.name), b.insert(b.end(), e.local_extra.begin(), e.local_extra.end());
        pl->body.push_back(b.size());
        b.insert(b.end(), e.body.begin(), e.body.end());
    }
    pl->cd_off = b.size();
    for (size_t i = 0; i < ents.size(); i++) {
        const Ent &e = ents[i];
        Bytes x;
        if (e.saturate) {
            put16(x, 1), put16(x, 8 * (uint32_t)__builtin_popcount((unsigned)e.saturate));
            if (e.saturate & 1) put64(x, e.size);
            if (e.saturate & 2) put64(x, e.body.size());
            if (e.saturate & 4) put64(x, pl->local[i]);
        }
        x.insert(x.end(), e.central_extra.begin(), e.central_extra.end());
        pl->record.push_back(b.size());
        put32(b, kZipSigCentral), put16(b, 20), put16(b, 20), put16(b, (uint32_t)e.flags), put16(b, (uint32_t)e.method), put16(b, 0x6000 + (uint32_t)i), put16(b, 0x21);
        put32(b, 0x11223344u), put32(b, e.saturate & 2 ? 0xFFFFFFFFu : (uint32_t)e.body.size()), put32(b, e.saturate & 1 ? 0xFFFFFFFFu : e.size);
        put16(b, (uint32_t)e.name.size()), put16(b, (uint32_t)x.size()), put16(b, 0), put16(b, 0), put16(b, 0), put32(b, 0x81A40000u);
        put32(b, e.saturate & 4 ? 0xFFFFFFFFu : (uint32_t)pl->local[i]);
        puts_(b, e.name), b.insert(b.end(), x.begin(), x.end());
    }
    pl->cd_len = b.size() - pl->cd_off;
    const uint32_t n = (uint32_t)ents.size();
    if (o.end64) {
        pl->end64 = b.size();
        put32(b, kZipSigEnd64), put64(b, 44), put16(b, 45), put16(b, 45), put32(b, 0), put32(b, 0), put64(b, n), put64(b, n), put64(b, pl->cd_len), put64(b, pl->cd_off);
        put32(b, kZipSigLocator), put32(b, 0), put64(b, pl->end64), put32(b, 1);
    }
    pl->end = b.size();
    put32(b, kZipSigEnd), put16(b, 0), put16(b, 0), put16(b, o.end64 ? 0xFFFF : n), put16(b, o.end64 ? 0xFFFF : n);
    put32(b, o.end64 ? 0xFFFFFFFFu : (uint32_t)pl->cd_len), put32(b, o.end64 ? 0xFFFFFFFFu : (uint32_t)pl->cd_off), put16(b, (uint32_t)o.comment.size());
    puts_(b, o.comment);
    if (!o.prefix.empty()) {
        const size_t k = o.prefix.size();
        b.insert(b.begin(), o.prefix.begin(), o.prefix.end());
        for (size_t &v : pl->local) v += k;
        for (size_t &v : pl->body) v += k;
        for (size_t &v : pl->record) v += k;
        pl->cd_off += k, pl->end += k;
        if (o.end64) pl->end64 += k;
    }
    return b;
}

static std::vector<Ent> three() {
    std::vector<Ent> v(3);
    v[0].name = "a.txt", v[0].method = 8, v[0].size = 50, v[0].body = Bytes(20, 0xAA);
    v[1].name = "b.bin", v[1].method = 0, v[1].size = 10, v[1].body = Bytes(10, 0xBB);
    v[2].name = "c/d.txt", v[2].method = 8, v[2].size = 7, v[2].body = Bytes(9, 0xCC);
    return v;
}

struct Walk {
    int rc;
    ZipInfo info;
    std::vector<ZipEntry> e;
    std::vector<uint8_t> why;
};
// the walk over a heap block of exactly the archive's bytes
static Walk walk(const Bytes &b, size_t len) {
    uint8_t *blk = (uint8_t *)malloc(len ? len : 1);
    if (len) memcpy(blk, b.data(), len);
    Walk w;
    w.rc = zip_find_end(blk, (int64_t)len, &w.info);
    if (w.rc == kZipOk) {
        w.e.resize((size_t)w.info.n_entries + 1), w.why.resize((size_t)w.info.n_entries + 1);
        w.rc = zip_walk(blk, (int64_t)len, &w.info, w.e.data(), w.info.n_entries, w.why.data());
        w.e.resize((size_t)w.info.n_entries), w.why.resize((size_t)w.info.n_entries);
    }
    free(blk);
    return w;
}
static Walk walk(const Bytes &b) { return walk(b, b.size()); }

// whole: walks, with every entry decodable where all_ok; cut anywhere: does not
static void every_prefix(const Bytes &b, const char *what, bool all_ok) {
    const Walk w = walk(b);
    CHECK(w.rc == kZipOk, "%s: %d", what, w.rc);
    for (size_t i = 0; i < w.why.size(); i++) CHECK(!all_ok || w.why[i] == kZipOk, "%s: entry %d: %d", what, (int)i, w.why[i]);
    for (size_t cut = 0; cut < b.size(); cut++) {
        const Walk c = walk(b, cut);
        CHECK(c.rc != kZipOk, "%s cut at %d walks", what, (int)cut);
        CHECK(cut >= (size_t)kZipEndBytes || c.rc == kZipShortFile, "%s cut at %d: %d", what, (int)cut, c.rc);
    }
}

static void expect_entry(const Bytes &b, int which, int why, const char *what) {
    const Walk w = walk(b);
    CHECK(w.rc == kZipOk && w.e.size() == 3, "%s: %d", what, w.rc);
    if (w.rc != kZipOk || w.e.size() != 3) return;
    for (int i = 0; i < 3; i++) {
        CHECK(w.why[(size_t)i] == (i == which ? why : (int)kZipOk), "%s: entry %d: %d", what, i, w.why[(size_t)i]);
        CHECK(w.e[(size_t)i].status == zip_err_status(w.why[(size_t)i]), "%s: entry %d: status %d", what, i, w.e[(size_t)i].status);
    }
}
static void expect_file(const Bytes &b, int rc, const char *what) {
    const Walk w = walk(b);
    CHECK(w.rc == rc, "%s: %d, not %d", what, w.rc, rc);
}

int main(int argc, char **argv) {
    // ---- archives from outside, whole and cut
    for (int a = 1; a < argc; a++) {
        FILE *fp = fopen(argv[a], "rb");
        if (!fp) {
            printf("FAIL cannot open %s\n", argv[a]);
            return 1;
        }
        Bytes b;
        for (int ch; (ch = fgetc(fp)) != EOF;) b.push_back((uint8_t)ch);
        fclose(fp);
        every_prefix(b, argv[a], true);
    }
    Places p;
    const std::vector<Ent> base = three();
    const Bytes good = build(base, Opt(), &p);
    // ---- the legal archive: what the walk says about it
    {
        every_prefix(good, "the plain archive", true);
        const Walk w = walk(good);
        CHECK(w.info.n_entries == 3 && w.info.total_len == 67 && w.info.shift == 0 && !w.info.zip64, "info");
        CHECK(w.info.cd_off == (int64_t)p.cd_off && w.info.cd_len == (int64_t)p.cd_len && w.info.comment_off == (int64_t)good.size() && w.info.comment_len == 0, "info places");
        const int64_t offs[3] = {0, 50, 60};
        for (size_t i = 0; i < 3 && i < w.e.size(); i++) {
            const ZipEntry &e = w.e[i];
            CHECK(e.local_off == (int64_t)p.local[i] && e.body_off == (int64_t)p.body[i] && e.out_off == offs[i], "entry %d places", (int)i);
            CHECK(e.name_off == (int64_t)p.record[i] + 46 && e.name_len == (int)base[i].name.size() && e.method == base[i].method, "entry %d name", (int)i);
            CHECK(e.len == base[i].size && e.comp_len == (int64_t)base[i].body.size() && e.crc32 == 0x11223344u && e.dos_time == 0x6000 + i && e.dos_date == 0x21 &&
                      e.external_attr == 0x81A40000u && e.status == 0,
                  "entry %d fields", (int)i);
        }
    }
    // ---- the end record
    {
        Opt o;
        o.comment = "a comment";
        Places q;
        Bytes b = build(base, o, &q);
        every_prefix(b, "with a comment", true);
        CHECK(walk(b).info.comment_len == 9 && walk(b).info.comment_off == (int64_t)q.end + 22, "comment");
        o.comment = std::string("PK\5\6", 4) + std::string(40, 'x') + std::string("PK\5\6", 4) + "tail";  // signatures in the comment, one with 22 bytes behind it
        b = build(base, o, &q);
        const Walk w = walk(b);
        CHECK(w.rc == kZipOk && w.info.n_entries == 3 && w.info.comment_len == 52, "a comment that holds the signature: %d", w.rc);
        Bytes c = b;
        poke16(c, q.end + 20, 51);  // the comment length one short: the record no longer reaches the end of the file
        expect_file(c, kZipNoEnd, "comment length one short");
        c = b, c.push_back(0);
        expect_file(c, kZipNoEnd, "a byte behind the comment");
        c = good, c[p.end] = 'Q';
        expect_file(c, kZipNoEnd, "no signature");
        c = good, poke16(c, p.end + 4, 1);
        expect_file(c, kZipMultiDisk, "disk 1");
        c = good, poke16(c, p.end + 6, 1);
        expect_file(c, kZipMultiDisk, "directory on disk 1");
        c = good, poke16(c, p.end + 8, 2);
        expect_file(c, kZipMultiDisk, "2 of 3 entries on this disk");
        // the comment's far end: 65535 bytes are searched, one more is not
        o.comment = std::string(65535, 'c');
        b = build(base, o, &q);
        CHECK(walk(b).rc == kZipOk, "a comment of 65535 bytes");
    }
    // ---- ZIP64: the end record and its locator
    {
        Opt o;
        o.end64 = true;
        Places q;
        const Bytes b = build(base, o, &q);
        every_prefix(b, "with a ZIP64 end record", true);
        const Walk w = walk(b);
        CHECK(w.rc == kZipOk && w.info.zip64 == 1 && w.info.n_entries == 3 && w.info.cd_off == (int64_t)q.cd_off && w.info.cd_len == (int64_t)q.cd_len && w.info.shift == 0, "ZIP64 end");
        Bytes c = b;
        poke32(c, q.end64 + 56 + 16, 2);
        expect_file(c, kZipMultiDisk, "two disks in the locator");
        c = b, poke32(c, q.end64 + 56 + 4, 1);
        expect_file(c, kZipMultiDisk, "the ZIP64 record on disk 1");
        c = b, c[q.end64 + 56] = 'Q';  // no locator, and the end record is all ones: 65535 entries that are not there
        expect_file(c, kZipBadShift, "all ones without a locator");
        c = b, c[q.end64] = 'Q';  // a locator that leads to no record
        expect_file(c, kZipBadEnd64, "no ZIP64 record");
        c = b, poke32(c, q.end64 + 4, 43);
        expect_file(c, kZipBadEnd64, "a ZIP64 record of 43 bytes");
        c = b, poke32(c, q.end64 + 32, 4);  // the total count (the end record's two are both all ones: both come from here)
        expect_file(c, kZipMultiDisk, "ZIP64 counts differ");
        // a record with an extensible data sector does not stand right in front of its locator: the locator's offset finds it
        c = b, c.insert(c.begin() + (long)q.end64 + 56, 8, 0x5A), poke32(c, q.end64 + 4, 52);
        CHECK(walk(c).rc == kZipOk && walk(c).info.zip64 == 1 && walk(c).info.shift == 0 && walk(c).info.n_entries == 3, "a ZIP64 record of 64 bytes: %d", walk(c).rc);
        poke32(c, q.end64 + 56 + 8 + 8, (uint32_t)q.end64 + 1);
        expect_file(c, kZipBadEnd64, "a locator that points beside the record");
        // only the count all ones: the rest stands as the end record has it
        c = b, poke32(c, q.end + 12, (uint32_t)q.cd_len), poke32(c, q.end + 16, (uint32_t)q.cd_off);
        CHECK(walk(c).rc == kZipOk && walk(c).info.zip64 == 1, "count alone from the ZIP64 record");
        // prefixed: the shift comes from the ZIP64 record's place
        o.prefix = "8 bytes!";
        const Bytes d = build(base, o, &q);
        const Walk wd = walk(d);
        CHECK(wd.rc == kZipOk && wd.info.shift == 8 && wd.info.cd_off == (int64_t)q.cd_off && wd.e.size() == 3 && wd.e[2].body_off == (int64_t)q.body[2] && wd.why[2] == kZipOk,
              "prefixed ZIP64: %d shift %d", wd.rc, (int)wd.info.shift);
    }
    // ---- the ZIP64 extra field, in the specification's order
    for (int sat = 1; sat < 8; sat++) {
        std::vector<Ent> v = three();
        v[1].saturate = sat;
        v[1].central_extra = {0x55, 0x54, 1, 0, 9};  // another field behind it
        v[2].central_extra = {0x55, 0x54, 1, 0, 9};
        v[2].saturate = sat;
        Places q;
        Bytes b = build(v, Opt(), &q);
        char what[64];
        snprintf(what, sizeof what, "ZIP64 extra field %d", sat);
        expect_entry(b, -1, kZipOk, what);
        const Walk w = walk(b);
        if (w.e.size() == 3) CHECK(w.e[2].len == 7 && w.e[2].comp_len == 9 && w.e[2].local_off == (int64_t)q.local[2] && w.e[2].body_off == (int64_t)q.body[2], "%s values", what);
        Bytes c = b;
        poke16(c, q.record[1] + 46 + 5 + 2, 8 * (uint32_t)__builtin_popcount((unsigned)sat) - 1);  // the field one byte short of what is asked of it
        expect_file(c, kZipBadDirectory, what);
        c = b, poke16(c, q.record[1] + 46 + 5, 2);  // no such field: the all-ones values stand, and reach past the file
        CHECK(walk(c).rc == kZipOk && walk(c).why[1] != kZipOk, "%s without the field", what);
    }
    // ---- bytes in front
    {
        Opt o;
        o.prefix = "MZ stub.";
        Places q;
        const Bytes b = build(base, o, &q);
        every_prefix(b, "prefixed", true);
        const Walk w = walk(b);
        CHECK(w.info.shift == 8 && w.info.cd_off == (int64_t)q.cd_off && w.e.size() == 3 && w.e[1].local_off == (int64_t)q.local[1] && w.e[1].body_off == (int64_t)q.body[1], "shift 8");
        Bytes c = good;
        poke32(c, p.end + 16, (uint32_t)p.cd_off + 1);
        expect_file(c, kZipBadShift, "the directory would end behind the end record");
        c = good, poke32(c, p.end + 12, (uint32_t)p.end + 1);
        expect_file(c, kZipBadShift, "a directory longer than the file");
    }
    // ---- the directory
    {
        Bytes c = good;
        c[p.record[1]] = 'Q';
        expect_file(c, kZipBadDirectory, "a record's signature");
        c = good, poke16(c, p.record[2] + 28, 8);  // the last name one longer: it would reach the end record
        expect_file(c, kZipBadDirectory, "a name out of the directory");
        c = good, poke16(c, p.record[2] + 30, 1);
        expect_file(c, kZipBadDirectory, "an extra field out of the directory");
        c = good, poke16(c, p.record[2] + 32, 1);
        expect_file(c, kZipBadDirectory, "a comment out of the directory");
        c = good, poke16(c, p.record[0] + 32, 1);  // the first record one longer: the second's signature is not where it ends
        expect_file(c, kZipBadDirectory, "records that do not meet");
        c = good, poke16(c, p.end + 8, 2), poke16(c, p.end + 10, 2);
        expect_file(c, kZipBadDirectory, "a record behind the last counted one");
        c = good, poke16(c, p.end + 8, 4), poke16(c, p.end + 10, 4);
        expect_file(c, kZipBadDirectory, "a record too few");
        // a record's comment, and an extra field, that do fit
        std::vector<Ent> v = three();
        v[0].central_extra = {0x55, 0x54, 1, 0, 9};
        Places q;
        expect_entry(build(v, Opt(), &q), -1, kZipOk, "an extra field in the directory only");
    }
    // ---- the entries: the middle one fails, its neighbours do not
    {
        for (int bit : {0, 6, 13}) {
            Bytes c = good;
            poke16(c, p.record[1] + 8, 1u << bit), poke16(c, p.local[1] + 6, 1u << bit);
            expect_entry(c, 1, kZipEncrypted, "an encryption flag");
        }
        for (int bit : {1, 2, 3, 4, 5, 11}) {  // (bit 3: a data descriptor, which nobody reads)
            Bytes c = good;
            poke16(c, p.record[1] + 8, 1u << bit), poke16(c, p.local[1] + 6, 1u << bit);
            expect_entry(c, -1, kZipOk, "a legal flag");
        }
        for (int method : {1, 7, 9, 12, 14, 93, 99}) {
            Bytes c = good;
            poke16(c, p.record[1] + 10, (uint32_t)method);
            expect_entry(c, 1, kZipBadMethod, "a method outside {0, 8}");
        }
        Bytes c = good;
        poke16(c, p.record[1] + 10, 8);  // (the same ten bytes as a deflated entry of other lengths: the walk decodes nothing)
        expect_entry(c, -1, kZipOk, "method 8");
        c = good, poke32(c, p.record[1] + 24, 11);
        expect_entry(c, 1, kZipStoredLength, "stored, len one more than comp_len");
        c = good, poke32(c, p.record[1] + 20, 9);
        expect_entry(c, 1, kZipStoredLength, "stored, comp_len one less than len");
        c = good, c[p.local[1] + 3] = 5;
        expect_entry(c, 1, kZipLocalMismatch, "the local signature");
        c = good, poke32(c, p.record[1] + 42, (uint32_t)p.local[1] + 1);
        expect_entry(c, 1, kZipLocalMismatch, "a local offset one off");
        c = good, poke16(c, p.local[1] + 26, 4);
        expect_entry(c, 1, kZipLocalMismatch, "the local name one shorter");
        c = good, c[p.local[1] + 30 + 2] ^= 1;
        expect_entry(c, 1, kZipLocalMismatch, "a local name byte");
        c = good, c[p.record[1] + 46 + 2] ^= 1;
        expect_entry(c, 1, kZipLocalMismatch, "a central name byte");
        c = good, poke32(c, p.record[2] + 20, (uint32_t)(good.size() - p.body[2]) + 1);
        expect_entry(c, 2, kZipTruncated, "a body one byte past the file");
        c = good, poke32(c, p.record[2] + 20, (uint32_t)(good.size() - p.body[2]));
        expect_entry(c, -1, kZipOk, "a body up to the last byte of the file");
        c = good, poke32(c, p.record[2] + 42, (uint32_t)good.size() - 3);
        expect_entry(c, 2, kZipTruncated, "a local header that the file ends in");
        // the local extra field moves the body, the central one does not
        std::vector<Ent> v = three();
        v[1].local_extra = Bytes(20, 0x77), v[1].central_extra = {0x55, 0x54, 1, 0, 9};
        Places q;
        c = build(v, Opt(), &q);
        expect_entry(c, -1, kZipOk, "a local extra field");
        CHECK(walk(c).e[1].body_off == (int64_t)q.local[1] + 30 + 5 + 20, "body behind the local extra field");
        // the sizes of a data descriptor entry are zero in the local header only
        c = good, poke16(c, p.record[0] + 8, 8), poke16(c, p.local[0] + 6, 8), poke32(c, p.local[0] + 14, 0), poke32(c, p.local[0] + 18, 0), poke32(c, p.local[0] + 22, 0);
        expect_entry(c, -1, kZipOk, "a data descriptor entry");
        CHECK(walk(c).e[0].len == 50 && walk(c).e[0].comp_len == 20 && walk(c).e[0].crc32 == 0x11223344u, "its sizes are the directory's");
    }
    // ---- no entries at all; and the smallest files
    {
        Places q;
        const Bytes b = build(std::vector<Ent>(), Opt(), &q);
        CHECK(b.size() == 22, "the empty archive");
        every_prefix(b, "the empty archive", true);
        CHECK(walk(b).info.n_entries == 0 && walk(b).info.total_len == 0, "the empty archive's counts");
    }
    // ---- the writer's records, read back
    {
        const std::string names[2] = {"one", "two/three.txt"};
        const int methods[2] = {kZipDeflated, kZipStored};
        const uint32_t comp[2] = {17, 5}, size[2] = {40, 5}, attr[2] = {0x81A40000u, 0x20};
        Bytes b, cd;
        uint32_t local_off[2];
        for (int i = 0; i < 2; i++) {
            local_off[i] = (uint32_t)b.size();
            b.resize(b.size() + 30);
            zip_put_local(b.data() + local_off[i], methods[i], i, 0x1234, 0x5678, comp[i], size[i], (uint32_t)names[i].size());
            puts_(b, names[i]), b.resize(b.size() + comp[i], 0xEE);
            const size_t r = cd.size();
            cd.resize(r + 46);
            zip_put_central(cd.data() + r, methods[i], i, 0x1234, 0x5678, comp[i], size[i], (uint32_t)names[i].size(), attr[i], local_off[i]);
            puts_(cd, names[i]);
        }
        const uint32_t cd_off = (uint32_t)b.size();
        b.insert(b.end(), cd.begin(), cd.end());
        b.resize(b.size() + 22);
        zip_put_eocd(b.data() + b.size() - 22, 2, (uint32_t)cd.size(), cd_off);
        every_prefix(b, "the writer's archive", true);
        const Walk w = walk(b);
        CHECK(w.rc == kZipOk && w.e.size() == 2 && w.info.cd_off == cd_off && w.info.total_len == 45, "the writer's archive");
        for (size_t i = 0; i < w.e.size(); i++) {
            const ZipEntry &e = w.e[i];
            CHECK(e.method == methods[i] && e.flags == (i ? 0x800 : 0) && e.crc32 == 0 && e.comp_len == comp[i] && e.len == size[i] && e.local_off == local_off[i] &&
                      e.body_off == (int64_t)local_off[i] + 30 + (int64_t)names[i].size() && e.dos_time == 0x1234 && e.dos_date == 0x5678 && e.external_attr == attr[i],
                  "the writer's entry %d", (int)i);
            CHECK(zip_le16(b.data() + local_off[i] + 4) == (i ? 10u : 20u) && zip_le16(b.data() + cd_off + (i ? 46 + 3 : 0) + 4) == (i ? 20u : (3u << 8 | 20u)), "versions of entry %d", (int)i);
        }
        CHECK(zip_bound(zip_entry_bound(zip_body_bound(5, kZipStored, 0), 13) + zip_entry_bound(zip_body_bound(40, kZipAuto, 0), 3)) == (int64_t)(22 + 76 + 26 + 5 + 76 + 6 + 40), "bound");
        CHECK(zip_body_bound(40, kZipDeflated, 1069) == 1063 && zip_body_bound(0, kZipDeflated, 1024) == 0, "a forced deflated body's bound");
    }
    printf("%s: %d checks, %d failed\n", fails ? "FAIL" : "PASS", checks, fails);
    return fails ? 1 : 0;
}
