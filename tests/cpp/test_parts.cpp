// The rules that the container calls share (zlibstream_amd/csrc/zs_parts.h) on the host: the staging layout, the 16-byte
// split of a sub-stream's place, the zlib header check against a restatement of its five branches, the verdict on an inflated
// sub-stream against the outcomes of the ZIP, TIFF and OpenEXR calls' own branches, the roll-up of codes and messages with
// both pairs of nouns, and which outputs of an encode call fit.
// Stand-alone: g++ -std=c++17 -Wall -fsanitize=address,undefined tests/cpp/test_parts.cpp && ./a.out
#include <cstdio>
#include <string>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_parts.h"

using namespace zs;

namespace {
int failures = 0, checks = 0;
void expect(bool ok, const std::string &what) {
    checks++;
    if (!ok) failures++, printf("FAIL: %s\n", what.c_str());
}

// InfMsg as zs_inflate.hip numbers it (zs_parts_host.inc asserts that zs_parts.h's names agree with the enum itself)
enum { kBadMethod = 1, kBadWindow = 2, kBadHeaderCheck = 3, kNeedDict = 4, kBadBlockType = 5, kTruncated = 18, kOutputFull = 19, kBadCheck = 20, kBadLength = 23 };

void test_layout() {
    const int64_t limit = 1000;
    const std::vector<int64_t> len{0, 1, 255, 256, 257, 1000, 1001, 5, 1 << 20, 0, 700};
    const StageLayout lay((int)len.size(), len.data(), limit);
    expect(lay.at.size() == len.size(), "layout: an offset per item");
    size_t end = 0;  // where the last staged item's room ends
    for (size_t i = 0; i < len.size(); i++) {
        expect(lay.at[i] % 256 == 0, "layout: offset " + std::to_string(i) + " is a multiple of 256");
        expect(lay.at[i] == end, "layout: item " + std::to_string(i) + " begins where the room before it ends");
        const bool room = len[i] > 0 && len[i] <= limit;
        expect(lay.staged(len[i]) == room, "layout: staged() of item " + std::to_string(i));
        if (room) {
            expect(lay.at[i] + (size_t)len[i] <= lay.at[i] + pad256((size_t)len[i]), "layout: the item fits its room");
            end = lay.at[i] + pad256((size_t)len[i]);
        }
        // an over-limit item and an empty one take no room: the next item has the same offset
        if (!room && i + 1 < len.size()) expect(lay.at[i + 1] == lay.at[i], "layout: item " + std::to_string(i) + " takes no room");
    }
    expect(lay.total == end && lay.total % 256 == 0, "layout: the total is the end of the last room");
    expect(lay.total == 256 * (1 + 1 + 1 + 2 + 4 + 1 + 3), "layout: the total of the staged items' rooms");
    StageLayout grown(limit);
    for (int64_t l : len) grown.add(l);
    expect(grown.at == lay.at && grown.total == lay.total, "layout: item by item gives the same layout");
    expect(pad256(0) == 0 && pad256(1) == 256 && pad256(256) == 256 && pad256(257) == 512, "pad256");
    expect(pad256(((size_t)1 << 40) + 1) == ((size_t)1 << 40) + 256, "pad256 above 2^32");
}

void test_split() {
    for (int skip : {0, 2})
        for (size_t file_at : {(size_t)0, (size_t)256, ((size_t)5 << 32) + 512})
            for (size_t off = 0; off < 48; off++)
                for (int64_t comp_len : {(int64_t)0, (int64_t)2, (int64_t)17, (int64_t)70000}) {
                    const size_t pos = file_at + off;
                    const SubStream ss = sub_stream(pos, comp_len, skip);
                    const std::string at = " (position " + std::to_string(pos) + ", skip " + std::to_string(skip) + ")";
                    expect(ss.base % 16 == 0 && ss.base <= pos && pos - ss.base < 16, "split: the base is the position rounded down to 16" + at);
                    expect(ss.base + (size_t)ss.body_off - (size_t)skip == pos, "split: base + body_off - skip is the position" + at);
                    expect(ss.base + (size_t)ss.in_len == pos + (size_t)comp_len, "split: in_len ends with the part" + at);
                }
    expect(sub_stream(33, 10).body_off == 1 && sub_stream(33, 10, 2).body_off == 3, "split: the header skip is added to the offset");
}

// The five branches as the TIFF call had them before they moved, restated
void old_head_check(const uint8_t *z, int64_t comp_len, int *status, int *msg) {
    *status = ZS_OK, *msg = 0;
    if (comp_len < 2) *status = ZS_BUF_ERROR, *msg = kTruncated;
    else if ((z[0] & 15) != 8) *status = ZS_DATA_ERROR, *msg = kBadMethod;
    else if ((z[0] >> 4) > 7) *status = ZS_DATA_ERROR, *msg = kBadWindow;
    else if (((z[0] << 8) | z[1]) % 31) *status = ZS_DATA_ERROR, *msg = kBadHeaderCheck;
    else if (z[1] & 0x20) *status = ZS_NEED_DICT, *msg = kNeedDict;
}
void test_head() {
    int seen[5] = {0, 0, 0, 0, 0}, passed = 0;
    for (int h = 0; h < 65536; h++) {
        const uint8_t z[2] = {(uint8_t)(h >> 8), (uint8_t)h};
        int want_st, want_msg, st = 77, msg = 77;
        old_head_check(z, 2, &want_st, &want_msg);
        const bool ok = zlib_head_check(z, 2, &st, &msg);
        if (want_st == ZS_OK) {
            passed++;
            expect(ok && st == 77 && msg == 77, "head " + std::to_string(h) + " passes and leaves the outputs alone");
        } else {
            expect(!ok && st == want_st && msg == want_msg, "head " + std::to_string(h) + " fails as before");
            seen[want_msg == kBadMethod ? 0 : want_msg == kBadWindow ? 1 : want_msg == kBadHeaderCheck ? 2 : want_msg == kNeedDict ? 3 : 4]++;
        }
        // a longer chunk changes nothing
        int st3 = 77, msg3 = 77;
        expect(zlib_head_check(z, 1 << 20, &st3, &msg3) == ok && (ok || (st3 == st && msg3 == msg)), "head " + std::to_string(h) + " at another length");
    }
    expect(passed > 0 && seen[0] > 0 && seen[1] > 0 && seen[2] > 0 && seen[3] > 0, "head: every branch is reached");
    const uint8_t good[2] = {0x78, 0x9C};
    for (int64_t len : {(int64_t)0, (int64_t)1}) {
        int st = 77, msg = 77;
        expect(!zlib_head_check(good, len, &st, &msg) && st == ZS_BUF_ERROR && msg == kTruncated, "head: " + std::to_string(len) + " bytes are too short");
        st = 77, msg = 77;
        expect(!zlib_head_check(nullptr, len, &st, &msg) && st == ZS_BUF_ERROR, "head: a short chunk's bytes are not read");
    }
    int st = 77, msg = 77;
    expect(zlib_head_check(good, 2, &st, &msg), "head: 78 9C passes");
}

// What the three calls did with one inflated sub-stream before the verdict moved, branch by branch.  Outcome: 'C' the call
// failed, 'F' the part failed with (code, msg), 'T' the part ends inside its Adler-32 (TIFF, OpenEXR), 'D' decoded.
struct Outcome {
    char kind;
    int code, msg;
};
Outcome old_outcome(bool zip, PartLenRule rule, int status, int msg, int64_t out_len, int64_t want, int64_t used, int64_t comp_len) {
    if (status == ZS_STREAM_ERROR || status == ZS_OK) return {'C', ZS_STREAM_ERROR, 0};
    if (status != ZS_STREAM_END) {
        const bool too_long = msg == kOutputFull;
        return {'F', too_long ? (int)ZS_DATA_ERROR : status, too_long ? (int)kBadLength : msg};
    }
    if (rule == kLenExact ? out_len != want : rule == kLenAtLeast ? out_len < want : false) return {'F', ZS_DATA_ERROR, kBadLength};
    if (!zip && used + 4 > comp_len) return {'T', ZS_BUF_ERROR, kTruncated};
    return {'D', ZS_OK, 0};
}
void test_verdict() {
    struct St {
        int status, msg;
    };
    // every status the inflate call writes, with the messages that matter: any other, and the one that is mapped
    const std::vector<St> sts{{ZS_STREAM_END, 0},          {ZS_STREAM_ERROR, 0},           {ZS_OK, 0},
                              {ZS_DATA_ERROR, kBadBlockType}, {ZS_DATA_ERROR, kBadCheck},     {ZS_BUF_ERROR, kTruncated},
                              {ZS_BUF_ERROR, kOutputFull},  {ZS_NEED_DICT, kNeedDict},      {ZS_MEM_ERROR, 0}};
    const int64_t want = 1000, comp_len = 300;
    int rows = 0, kinds[4] = {0, 0, 0, 0};
    for (PartLenRule rule : {kLenAny, kLenExact, kLenAtLeast})
        for (bool zip : {false, true})
            for (const St &s : sts)
                for (int64_t out_len : {want - 1, want, want + 1})
                    for (int64_t used : {comp_len - 5, comp_len - 4, comp_len - 3, comp_len}) {
                        const Outcome o = old_outcome(zip, rule, s.status, s.msg, out_len, want, used, comp_len);
                        const PartVerdict v = part_verdict(s.status, s.msg, out_len, used, comp_len, rule, want);
                        // the callers' use of the verdict: ZIP does not look at the trailer
                        Outcome got{'D', ZS_OK, 0};
                        if (v.cls == kPartCallFailed) got = {'C', ZS_STREAM_ERROR, 0};
                        else if (v.cls == kPartFailed) got = {'F', v.code, v.msg};
                        else if (!zip && v.trailer_cut) got = {'T', ZS_BUF_ERROR, kTruncated};
                        rows++, kinds[o.kind == 'C' ? 0 : o.kind == 'F' ? 1 : o.kind == 'T' ? 2 : 3]++;
                        expect(got.kind == o.kind && got.code == o.code && got.msg == o.msg,
                               "verdict: rule " + std::to_string(rule) + (zip ? " zip" : " zlib") + " status " + std::to_string(s.status) + " msg " + std::to_string(s.msg) + " out_len " +
                                   std::to_string(out_len) + " used " + std::to_string(used) + ": " + got.kind + " against " + o.kind);
                        if (v.cls != kPartDecoded) expect(!v.trailer_cut, "verdict: only a decoded part has a trailer to be cut");
                    }
    expect(rows == 3 * 2 * 9 * 3 * 4 && kinds[0] && kinds[1] && kinds[2] && kinds[3], "verdict: the table reaches every outcome");
    // the rows that name the rules
    PartVerdict v = part_verdict(ZS_BUF_ERROR, kOutputFull, want, 0, comp_len, kLenExact, want);
    expect(v.cls == kPartFailed && v.code == ZS_DATA_ERROR && v.msg == kBadLength, "verdict: out of room is a wrong length");
    v = part_verdict(ZS_BUF_ERROR, kTruncated, 10, 0, comp_len, kLenExact, want);
    expect(v.cls == kPartFailed && v.code == ZS_BUF_ERROR && v.msg == kTruncated, "verdict: any other failure keeps its code and message");
    v = part_verdict(ZS_STREAM_END, 0, want + 1, 10, comp_len, kLenAtLeast, want);
    expect(v.cls == kPartDecoded && !v.trailer_cut, "verdict: at-least accepts a longer part");
    v = part_verdict(ZS_STREAM_END, 0, want + 1, 10, comp_len, kLenExact, want);
    expect(v.cls == kPartFailed && v.code == ZS_DATA_ERROR && v.msg == kBadLength, "verdict: exact refuses a longer part");
    v = part_verdict(ZS_STREAM_END, 0, 3, 10, comp_len, kLenAny, want);
    expect(v.cls == kPartDecoded, "verdict: no rule, any length");
    v = part_verdict(ZS_STREAM_END, 0, want, comp_len - 3, comp_len, kLenExact, want);
    expect(v.cls == kPartDecoded && v.trailer_cut, "verdict: three bytes behind the last block are no Adler-32");
    int code = 0, why = 0;
    part_failure(ZS_BUF_ERROR, kOutputFull, &code, &why);
    expect(code == ZS_DATA_ERROR && why == kBadLength, "part_failure maps the full output");
    part_failure(ZS_DATA_ERROR, kBadCheck, &code, &why);
    expect(code == ZS_DATA_ERROR && why == kBadCheck, "part_failure keeps the rest");
}

// The roll-up as the four calls had it before it moved: "%d" for the numbers, the nouns in the format strings
int old_roll_up(const char *file_fmt, const char *part_fmt, std::vector<int> &st, std::vector<std::string> &why, const std::vector<std::vector<int>> &cst,
                const std::vector<std::vector<const char *>> &cwhy, int *const *part_status, const std::string &before, std::string *err) {
    const int n = (int)st.size();
    for (int i = 0; i < n; i++) {
        if (st[(size_t)i] != ZS_OK) continue;
        if (part_status && part_status[i] && !cst[(size_t)i].empty()) memcpy(part_status[i], cst[(size_t)i].data(), sizeof(int) * cst[(size_t)i].size());
        for (size_t k = 0; k < cst[(size_t)i].size(); k++)
            if (cst[(size_t)i][k] != ZS_OK) {
                char head[48];
                snprintf(head, sizeof head, part_fmt, (int)k);
                st[(size_t)i] = cst[(size_t)i][k], why[(size_t)i] = std::string(head) + cwhy[(size_t)i][k];
                break;
            }
    }
    *err = before;
    for (int i = 0; i < n; i++)
        if (st[(size_t)i] != ZS_OK) {
            char head[48];
            snprintf(head, sizeof head, file_fmt, i);
            *err = std::string(head) + why[(size_t)i];
            return st[(size_t)i];
        }
    return ZS_OK;
}

struct Fail {
    int file;
    int part;  // -1: the whole file
    int code;
    const char *text;
};
void roll_case(const std::string &name, const std::vector<Fail> &fails, int want_rc, const std::string &want_entry, const std::string &want_chunk,
               const std::string &want_array, const std::vector<int> &want_st) {
    const size_t parts_of[3] = {0, 1, 3};
    const struct {
        const char *file, *part, *file_fmt, *part_fmt;
        const std::string *want;
    } nouns[3] = {{"file", "entry", "file %d: ", "entry %d: ", &want_entry}, {"file", "chunk", "file %d: ", "chunk %d: ", &want_chunk},
                  {"array", "chunk", "array %d: ", "chunk %d: ", &want_array}};
    std::vector<bool> whole(3, false);  // the file is refused as a whole: it has no parts
    for (const Fail &f : fails)
        if (f.part < 0) whole[(size_t)f.file] = true;
    auto fill = [&](PartCodes &pc) {
        for (int i = 0; i < 3; i++)
            if (!whole[(size_t)i]) pc.open_parts(i, parts_of[i]);
        for (const Fail &f : fails) f.part < 0 ? pc.fail_file(f.file, f.code, f.text) : pc.fail_part(f.file, f.part, f.code, f.text);
    };
    for (const auto &nn : nouns) {
        const std::string tag = "roll_up (" + name + ", " + nn.file + " / " + nn.part + "): ";
        std::vector<int> st(3, ZS_OK), old_st(3, ZS_OK);
        PartCodes pc(st);
        fill(pc);
        std::vector<std::string> old_why(3);
        std::vector<std::vector<int>> old_cst(3);
        std::vector<std::vector<const char *>> old_cwhy(3);
        for (int i = 0; i < 3; i++)
            if (!whole[(size_t)i]) old_cst[(size_t)i].assign(parts_of[i], ZS_OK), old_cwhy[(size_t)i].assign(parts_of[i], "");
        for (const Fail &f : fails) {
            if (f.part >= 0) old_cst[(size_t)f.file][(size_t)f.part] = f.code, old_cwhy[(size_t)f.file][(size_t)f.part] = f.text;
            else if (old_st[(size_t)f.file] == ZS_OK) old_st[(size_t)f.file] = f.code, old_why[(size_t)f.file] = f.text;
        }
        int got_parts[3][3], old_parts[3][3];
        for (auto &row : got_parts) row[0] = row[1] = row[2] = 99;
        memcpy(old_parts, got_parts, sizeof got_parts);
        int *const got_ptr[3] = {got_parts[0], got_parts[1], got_parts[2]}, *const old_ptr[3] = {old_parts[0], old_parts[1], old_parts[2]};
        std::string err = "left by an inner call", old_err = err;
        const int rc = pc.roll_up(nn.file, nn.part, got_ptr, "before", &err);
        const int old_rc = old_roll_up(nn.file_fmt, nn.part_fmt, old_st, old_why, old_cst, old_cwhy, old_ptr, "before", &old_err);
        expect(rc == old_rc && err == old_err && st == old_st && pc.why == old_why, tag + "the code, the message and the files' codes are the earlier roll-up's (\"" + err + "\")");
        expect(memcmp(got_parts, old_parts, sizeof got_parts) == 0, tag + "the parts' codes are copied out as before");
        expect(rc == want_rc && err == *nn.want && st == want_st, tag + "got \"" + err + "\", want \"" + *nn.want + "\"");
        for (int i = 0; i < 3; i++)
            for (size_t k = 0; k < 3; k++)
                expect((got_parts[i][k] != 99) == (!whole[(size_t)i] && k < parts_of[i]), tag + "part codes of file " + std::to_string(i) + " leave only where the file was accepted");
        for (const Fail &f : fails)
            if (f.part >= 0 && !whole[(size_t)f.file]) expect(got_parts[f.file][f.part] == f.code, tag + "a failing part's code is in the list");
        // part codes wanted for the last file only, and for none: nothing else changes
        int only2[3] = {99, 99, 99};
        int *const some[3] = {nullptr, nullptr, only2};
        for (int *const *ptr : {(int *const *)some, (int *const *)nullptr}) {
            std::vector<int> st2(3, ZS_OK);
            PartCodes pc2(st2);
            fill(pc2);
            std::string err2;
            expect(pc2.roll_up(nn.file, nn.part, ptr, "before", &err2) == rc && err2 == err && st2 == st, tag + "the same with fewer lists of part codes");
        }
        expect(whole[2] ? only2[0] == 99 : only2[0] == got_parts[2][0] && only2[2] == got_parts[2][2], tag + "the one list is the file's");
    }
}
void test_roll_up() {
    roll_case("nothing fails", {}, ZS_OK, "before", "before", "before", {ZS_OK, ZS_OK, ZS_OK});
    roll_case("a later part", {{2, 2, ZS_DATA_ERROR, "incorrect data check"}}, ZS_DATA_ERROR, "file 2: entry 2: incorrect data check", "file 2: chunk 2: incorrect data check",
              "array 2: chunk 2: incorrect data check", {ZS_OK, ZS_OK, ZS_DATA_ERROR});
    roll_case("two parts, the first wins", {{2, 2, ZS_DATA_ERROR, "incorrect data check"}, {2, 1, ZS_BUF_ERROR, "unexpected end of stream"}}, ZS_BUF_ERROR,
              "file 2: entry 1: unexpected end of stream", "file 2: chunk 1: unexpected end of stream", "array 2: chunk 1: unexpected end of stream", {ZS_OK, ZS_OK, ZS_BUF_ERROR});
    roll_case("the first failing file is the call's", {{2, 0, ZS_DATA_ERROR, "incorrect data check"}, {1, 0, ZS_NEED_DICT, "need dictionary"}}, ZS_NEED_DICT,
              "file 1: entry 0: need dictionary", "file 1: chunk 0: need dictionary", "array 1: chunk 0: need dictionary", {ZS_OK, ZS_NEED_DICT, ZS_DATA_ERROR});
    roll_case("a whole file", {{1, -1, ZS_BUF_ERROR, "buffer error"}, {2, 1, ZS_DATA_ERROR, "incorrect data check"}}, ZS_BUF_ERROR, "file 1: buffer error", "file 1: buffer error",
              "array 1: buffer error", {ZS_OK, ZS_BUF_ERROR, ZS_DATA_ERROR});
    roll_case("a whole file twice, the first stays", {{0, -1, ZS_DATA_ERROR, "the file is above 2 GiB - 1 KiB"}, {0, -1, ZS_BUF_ERROR, "buffer error"}}, ZS_DATA_ERROR,
              "file 0: the file is above 2 GiB - 1 KiB", "file 0: the file is above 2 GiB - 1 KiB", "array 0: the file is above 2 GiB - 1 KiB", {ZS_DATA_ERROR, ZS_OK, ZS_OK});
    // the gzip files call's end: no parts, and the message left alone where no file failed
    std::vector<int> st(3, ZS_OK);
    PartCodes pc(st);
    std::string err = "untouched";
    expect(pc.first_file("file", &err) == ZS_OK && err == "untouched", "first_file leaves the message where nothing failed");
    pc.fail_file(2, ZS_BUF_ERROR, "unexpected end of stream");
    pc.fail_file(2, ZS_DATA_ERROR, "later");
    expect(pc.first_file("file", &err) == ZS_BUF_ERROR && err == "file 2: unexpected end of stream", "first_file: \"" + err + "\"");
    // a file or part number with many digits: "%lld" prints what "%d" printed
    std::vector<int> big(1234568, ZS_OK);
    PartCodes pb(big);
    pb.open_parts(1234567, 2000000);
    pb.fail_part(1234567, 1999999, ZS_DATA_ERROR, "incorrect chunk length");
    expect(pb.roll_up("array", "chunk", nullptr, "before", &err) == ZS_DATA_ERROR && err == "array 1234567: chunk 1999999: incorrect chunk length", "roll_up digits: \"" + err + "\"");
}

void test_fit() {
    const int64_t len[4] = {10, 20, 30, 0}, roomy[4] = {10, 25, 30, 0}, tight[4] = {9, 20, 29, 0}, none[4] = {0, 0, 0, -1};
    {
        std::vector<int> st(4, ZS_OK);
        int rc = ZS_OK;
        std::string err = "before";
        expect(mark_fit(st, len, roomy, &rc, &err) == 4 && rc == ZS_OK && err == "before" && st == std::vector<int>(4, ZS_OK), "fit: all fit, nothing is touched");
    }
    {
        std::vector<int> st(4, ZS_OK);
        int rc = ZS_OK;
        std::string err = "before";
        expect(mark_fit(st, len, tight, &rc, &err) == 2 && rc == ZS_BUF_ERROR && err == "buffer error" && st == std::vector<int>({ZS_BUF_ERROR, ZS_OK, ZS_BUF_ERROR, ZS_OK}),
               "fit: some fit");
    }
    {
        std::vector<int> st(4, ZS_OK);
        int rc = ZS_OK;
        std::string err = "before";
        expect(mark_fit(st, len, none, &rc, &err) == 0 && rc == ZS_BUF_ERROR && err == "buffer error" && st == std::vector<int>(4, ZS_BUF_ERROR), "fit: none fits");
    }
    {
        // an output that has failed already is neither counted nor marked, and an earlier code of the call stays
        std::vector<int> st{ZS_STREAM_ERROR, ZS_OK, ZS_OK, ZS_OK};
        int rc = ZS_STREAM_ERROR;
        std::string err = "stream error";
        expect(mark_fit(st, len, tight, &rc, &err) == 2 && rc == ZS_STREAM_ERROR && err == "stream error" && st == std::vector<int>({ZS_STREAM_ERROR, ZS_OK, ZS_BUF_ERROR, ZS_OK}),
               "fit: behind an earlier failure");
    }
    std::vector<int> st{ZS_OK, ZS_BUF_ERROR, ZS_OK, ZS_DATA_ERROR};
    fail_live(st, ZS_MEM_ERROR);
    expect(st == std::vector<int>({ZS_MEM_ERROR, ZS_BUF_ERROR, ZS_MEM_ERROR, ZS_DATA_ERROR}), "fail_live leaves a failed output's code alone");
}
}  // namespace

int main() {
    test_layout();
    test_split();
    test_head();
    test_verdict();
    test_roll_up();
    test_fit();
    if (failures) return printf("%d of %d checks failed\n", failures, checks), 1;
    printf("PASS %d checks\n", checks);
    return 0;
}
