"""The host side of the ZIP calls, no GPU: the container rules of zlibstream_amd/csrc/zs_zip.h run by
tests/cpp/test_zip_walk.cpp under the address and undefined-behaviour sanitizers, zip_file_info against zipfile's own
infolist() on archives zipfile wrote and on hand-built ones (tests/zip_cases.py), every error class beside its legal
neighbour, zip_bound, and the argument checks of the two device calls that are decided before any device work."""
import ctypes
import io
import os
import struct
import subprocess
import zipfile
import zlib

import pytest

import zip_cases as zc
from zlibstream_amd import (ZIP_AUTO, ZIP_DEFLATED, ZIP_STORED, ZlibStreamException, _native, wrap_bound, WRAP_RAW, zip_bound, zip_file_info)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = open(os.path.join(ROOT, "tests", "golden", "corpus", "alice29.txt"), "rb").read()


class Unseekable(io.RawIOBase):
    """A stream zipfile cannot seek in: it writes data descriptors (flag bit 3) behind the bodies."""

    def __init__(self):
        self.buf = io.BytesIO()

    def writable(self):
        return True

    def write(self, b):
        return self.buf.write(b)


def written(fill, comment=b"", unseekable=False, **kw):
    """An archive written by zipfile: fill(z) adds the entries.  Returns (bytes, the ZipInfo list zipfile reads back from them
    -- from the same bytes without the comment, since zipfile takes the last end record signature it finds for the record)."""
    f = Unseekable() if unseekable else io.BytesIO()
    with zipfile.ZipFile(f, "w", **kw) as z:
        fill(z)
        z.comment = comment
    arch = (f.buf if unseekable else f).getvalue()
    bare = arch[:len(arch) - len(comment) - 2] + b"\0\0"
    with zipfile.ZipFile(io.BytesIO(bare)) as z:
        assert z.testzip() is None
        return arch, z.infolist()


def mixed(z):
    z.writestr(zipfile.ZipInfo("deflated.txt", (2024, 2, 29, 13, 14, 16)), TEXT[:5000], zipfile.ZIP_DEFLATED)
    z.writestr("stored.bin", bytes(range(256)) * 3, zipfile.ZIP_STORED)
    z.writestr("empty", b"", zipfile.ZIP_DEFLATED)
    z.writestr("a/directory/", b"")
    z.writestr("grüße.txt", TEXT[5000:5300], zipfile.ZIP_DEFLATED)


def forced64(z):
    for name, data, kind in (("one", TEXT[:700], zipfile.ZIP_DEFLATED), ("two", b"stored bytes", zipfile.ZIP_STORED)):
        zi = zipfile.ZipInfo(name)
        zi.compress_type = kind
        with z.open(zi, "w", force_zip64=True) as w:
            w.write(data)


def agrees(arch, infos, shift=0):
    """zip_file_info says what zipfile's infolist() says, and every entry is decodable."""
    info, ents = zip_file_info(arch)
    assert info["n_entries"] == len(infos) == len(ents) and info["shift"] == shift
    assert info["total_len"] == sum(i.file_size for i in infos)
    off = 0
    for e, i in zip(ents, infos):
        assert e["name"] == i.filename and e["method"] == i.compress_type and e["crc32"] == i.CRC and e["flags"] == i.flag_bits
        assert e["len"] == i.file_size and e["comp_len"] == i.compress_size and e["local_off"] == i.header_offset + shift
        assert e["out_off"] == off and e["status"] == 0 and e["external_attr"] == i.external_attr
        date = (e["dos_date"] >> 9) + 1980, e["dos_date"] >> 5 & 15, e["dos_date"] & 31, e["dos_time"] >> 11, e["dos_time"] >> 5 & 63, (e["dos_time"] & 31) * 2
        assert date == tuple(i.date_time[:5]) + (i.date_time[5] & ~1,)
        body = arch[e["body_off"]:e["body_off"] + e["comp_len"]]
        data = zlib.decompress(body, -15) if e["method"] == 8 else body
        assert len(data) == e["len"] and zlib.crc32(data) == e["crc32"]
        off += e["len"]
    return info, ents


def small_archives():
    plain, _ = written(mixed)
    z64, _ = written(forced64)
    dd, _ = written(mixed, unseekable=True)
    return plain, z64, dd


def test_shared_zip_rules_on_the_host_under_sanitizers():
    """tests/cpp/test_zip_walk.cpp, a stand-alone program built with -fsanitize=address,undefined: every prefix of three
    archives zipfile wrote (plain, force_zip64, data descriptors) and of the ones it builds, each in a heap block of exactly its
    length, and both sides of every rule."""
    build = os.path.join(ROOT, "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_zip_walk")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_zip_walk.cpp")], check=True)
    paths = []
    for k, arch in enumerate(small_archives()):
        paths.append(os.path.join(build, "test_zip_walk_%d.zip" % k))
        with open(paths[-1], "wb") as f:
            f.write(arch)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), (r.stdout[-2000:], r.stderr[-3000:])


def test_file_info_agrees_with_zipfile_on_its_own_archives():
    arch, infos = written(mixed)
    info, ents = agrees(arch, infos)
    assert [e["method"] for e in ents] == [8, 0, 8, 0, 8] and ents[2]["len"] == 0 and ents[3]["name"] == "a/directory/"
    assert info["zip64"] == 0 and info["comment_len"] == 0 and info["comment_off"] == len(arch)
    assert info["cd_off"] == infos[-1].header_offset + 30 + len(infos[-1].filename.encode()) + infos[-1].compress_size
    assert ents[4]["flags"] & 0x800 and ents[0]["dos_date"] == (44 << 9 | 2 << 5 | 29)
    # an archive comment, and one that holds the end record's signature (which zipfile itself could not read back)
    arch, infos = written(mixed, comment=b"about this archive")
    info, _ = agrees(arch, infos)
    assert arch[info["comment_off"]:info["comment_off"] + info["comment_len"]] == b"about this archive"
    for comment in (b"PK\5\6", b"x" * 30 + b"PK\5\6" + b"y" * 40, b"PK\5\6" * 20):
        arch, infos = written(mixed, comment=comment)
        info, _ = agrees(arch, infos)
        assert arch[info["comment_off"]:] == comment and info["comment_len"] == len(comment)
    # written to a stream that cannot seek: data descriptors, zeros in the local headers
    arch, infos = written(mixed, unseekable=True)
    _, ents = agrees(arch, infos)
    assert all(e["flags"] & 8 for e in ents) and struct.unpack_from("<III", arch, ents[0]["local_off"] + 14) == (0, 0, 0)
    with zipfile.ZipFile(io.BytesIO(arch)) as z:
        assert z.testzip() is None
    # force_zip64: a ZIP64 extra field in the local header only, which moves the body
    arch, infos = written(forced64)
    _, ents = agrees(arch, infos)
    assert [e["body_off"] - e["local_off"] for e in ents] == [30 + 3 + 20] * 2 and struct.unpack_from("<HH", arch, ents[0]["local_off"] + 33) == (1, 16)
    # eight bytes in front
    arch, infos = written(mixed)
    info, _ = agrees(b"\x7fELFjunk" + arch, infos, shift=8)
    assert info["cd_off"] == 8 + zip_file_info(arch)[0]["cd_off"]
    with zipfile.ZipFile(io.BytesIO(b"\x7fELFjunk" + arch)) as z:
        assert z.testzip() is None
    # no entries
    arch, infos = written(lambda z: None)
    assert agrees(arch, infos)[0]["total_len"] == 0 and len(arch) == 22


def test_file_info_of_hand_built_archives():
    places = {}
    ents = zc.three()
    arch = zc.legal(zc.archive(ents, places=places), ents)
    info, got = zip_file_info(arch)
    assert info == {"n_entries": 3, "total_len": sum(len(e["data"]) for e in ents), "cd_off": places["cd_off"], "cd_len": places["cd_len"], "shift": 0,
                    "comment_off": len(arch), "comment_len": 0, "zip64": 0}
    assert [g["local_off"] for g in got] == places["local_off"] and [g["body_off"] for g in got] == places["body_off"]
    assert [g["name"] for g in got] == ["first.txt", "mid.bin", "dir/last.txt"] and [g["status"] for g in got] == [0, 0, 0]
    # a ZIP64 end record, whole, prefixed, and with only some of the end record's fields all ones
    for prefix in (b"", b"12345678"):
        arch = zc.legal(zc.archive(ents, prefix=prefix, end64=True, places=places), ents)
        info, got = zip_file_info(arch)
        assert (info["zip64"], info["n_entries"], info["shift"], info["cd_off"], info["cd_len"]) == (1, 3, len(prefix), places["cd_off"], places["cd_len"])
        assert [g["body_off"] for g in got] == places["body_off"] and [g["status"] for g in got] == [0, 0, 0]
    # ZIP64 extra fields in the directory: each subset of the three fields, in the specification's order
    for sat in range(1, 8):
        places = {}
        plain = zc.archive(ents, places=places)
        e = ents[1]
        vals = [v for k, v in enumerate((len(e["data"]), len(e["body"]), places["local_off"][1])) if sat >> k & 1]
        ce = dict(extra=zc.zip64_extra(*vals))
        if sat & 1:
            ce["size"] = 0xFFFFFFFF
        if sat & 2:
            ce["comp_len"] = 0xFFFFFFFF
        if sat & 4:
            ce["local_off"] = 0xFFFFFFFF
        mid = dict(e, ce=ce)
        arch = zc.legal(zc.archive([ents[0], mid, ents[2]]), ents)
        got = zip_file_info(arch)[1]
        want = zip_file_info(plain)[1]
        for g, w in zip(got, want):
            assert {k: g[k] for k in ("len", "comp_len", "local_off", "body_off", "out_off", "status")} == {k: w[k] for k in ("len", "comp_len", "local_off", "body_off", "out_off", "status")}
    # counts only, and a list too short for the entries
    L = _native.lib()
    info = _native.ZipInfo()
    arch = zc.archive(ents)
    assert L.zs_zip_file_info(arch, len(arch), ctypes.byref(info), None, 0) == 0 and info.n_entries == 3 and info.total_len == sum(len(e["data"]) for e in ents)
    two = (_native.ZipEntry * 3)()
    two[2].status = 77
    assert L.zs_zip_file_info(arch, len(arch), ctypes.byref(info), two, 2) == -5 and info.n_entries == 3
    assert [two[k].len for k in range(2)] == [len(e["data"]) for e in ents[:2]] and two[2].status == 77
    assert L.zs_zip_file_info(None, 0, ctypes.byref(info), None, 0) == -2 and L.zs_zip_file_info(arch, -1, ctypes.byref(info), None, 0) == -2
    assert L.zs_zip_file_info(arch, len(arch), None, None, 0) == -2 and L.zs_zip_file_info(arch, len(arch), ctypes.byref(info), None, 1) == -2


def file_fails(arch, code):
    with pytest.raises(ZlibStreamException, match=r"\(%d\)" % code):
        zip_file_info(arch)


def test_file_level_errors_beside_the_legal_archive():
    ents = zc.three()
    places = {}
    good = zc.legal(zc.archive(ents, places=places), ents)
    end = places["end_off"]
    for cut in range(len(good)):
        file_fails(good[:cut], -5 if cut < 22 else -3)
    for field, val in ((4, 1), (6, 1), (8, 2)):  # this disk, the directory's disk, the entries on this disk
        b = bytearray(good)
        struct.pack_into("<H", b, end + field, val)
        file_fails(b, -3)
    file_fails(zc.archive(ents, end=dict(sig=b"PK\5\7")), -3)
    file_fails(zc.archive(ents, end=dict(comment_len=1)), -3)
    file_fails(good + b"\0", -3)
    zc.legal(zc.archive(ents, comment=b"\0"), ents)
    # the directory would begin in front of the file / a directory that is not where the end record says
    b = bytearray(good)
    struct.pack_into("<I", b, end + 16, places["cd_off"] + 1)
    file_fails(b, -3)
    # ZIP64: two disks, a locator without its record, all-ones fields without either
    arch = zc.archive(ents, end64=True)
    assert zip_file_info(arch)[0]["zip64"] == 1
    file_fails(zc.archive(ents, end64=True, end64_fields=dict(n_disks=2)), -3)
    file_fails(zc.archive(ents, end64=True, end64_fields=dict(sig=b"PK\6\5")), -3)
    file_fails(zc.archive(ents, end64=True, end64_fields=dict(loc_sig=b"PK\6\5")), -3)
    file_fails(zc.archive(ents, end64=True, end64_fields=dict(n_here=2)), -3)
    # the directory: a signature, lengths that leave it, its end, its count
    for k, mid in enumerate((dict(sig=b"PK\1\3"), dict(name_len=8), dict(extra_len=200), dict(comment_len=200))):
        file_fails(zc.archive([ents[0], dict(ents[1], ce=mid), ents[2]]), -3)
    for n in (2, 4):
        b = bytearray(good)
        struct.pack_into("<HH", b, end + 8, n, n)
        file_fails(b, -3)
    b = bytearray(good)
    struct.pack_into("<I", b, end + 12, places["cd_len"] - 1)  # (and the shift it implies finds no record)
    file_fails(b, -3)
    # a ZIP64 extra field too short for what the record asks of it
    file_fails(zc.archive([ents[0], dict(ents[1], ce=dict(size=0xFFFFFFFF, comp_len=0xFFFFFFFF, extra=zc.zip64_extra(len(ents[1]["data"])))), ents[2]]), -3)


ENTRY_CASES = {
    # name: (the middle entry's changes, code)
    "encrypted": (dict(flags=1), -3), "strong encryption": (dict(flags=1 << 6), -3), "masked directory": (dict(flags=1 << 13), -3),
    "method 12": (dict(ce=dict(method=12), lo=dict(method=12)), -3), "method 9": (dict(ce=dict(method=9)), -3),
    "stored lengths differ": (dict(ce=dict(size=201)), -3),
    "local signature": (dict(lo=dict(sig=b"PK\3\5")), -3), "local name length": (dict(lo=dict(name_len=6)), -3),
    "comp_len past the file": (dict(ce=dict(comp_len=1 << 20, size=1 << 20)), -5),
}


def test_entry_level_errors_beside_their_legal_neighbours():
    base = zc.three()
    zc.legal(zc.archive(base), base)
    assert [e["status"] for e in zip_file_info(zc.archive(base))[1]] == [0, 0, 0]
    for name, (change, code) in ENTRY_CASES.items():
        mid = dict(base[1])
        for k, v in change.items():
            mid[k] = dict(mid[k], **v) if isinstance(v, dict) else v
        arch = zc.archive([base[0], mid, base[2]])
        info, got = zip_file_info(arch)
        assert [e["status"] for e in got] == [0, code, 0], name
        assert info["total_len"] == sum(e["len"] for e in got) and got[2]["out_off"] == got[0]["len"] + got[1]["len"], name
    # another local name of the same length
    other = zc.archive([base[0], dict(base[1], name=b"MID.bin"), base[2]])
    places = {}
    good = zc.archive(base, places=places)
    at = places["local_off"][1]
    arch = good[:at] + other[at:at + 30 + 7] + good[at + 30 + 7:]
    assert [e["status"] for e in zip_file_info(arch)[1]] == [0, -3, 0] and len(arch) == len(good)
    # legal: a data descriptor flag, a local extra field the directory does not have, and a last body that ends the entries
    ok = [zc.entry(b"first.txt", base[0]["data"], descriptor=True), zc.entry(b"mid.bin", base[1]["data"], method=zc.STORED, local_extra=zc.zip64_extra(200, 200)), base[2]]
    arch = zc.legal(zc.archive(ok), ok)
    got = zip_file_info(arch)[1]
    assert [e["status"] for e in got] == [0, 0, 0] and got[0]["flags"] == 8 and got[1]["body_off"] == got[1]["local_off"] + 30 + 7 + 20
    # a local header that the file ends in: the last entry's offset moved to the last three bytes
    last = dict(base[2], ce=dict(local_off=len(good) - 3))
    assert [e["status"] for e in zip_file_info(zc.archive([base[0], base[1], last]))[1]] == [0, 0, -5]


def test_zip_bound():
    stored = [(b"a.bin", 256, 1000, ZIP_STORED), (b"dir/b", 0, 0, ZIP_STORED), (b"c" * 300, 256, 77, ZIP_STORED)]
    exact = 22 + sum(30 + 46 + 2 * len(n) + ln for n, _, ln, _ in stored)
    assert zip_bound(stored) == exact
    arch = io.BytesIO()
    with zipfile.ZipFile(arch, "w") as z:  # (what zipfile writes for the same stored entries: as long, byte for byte)
        for n, _, ln, _ in stored:
            z.writestr(zipfile.ZipInfo(n.decode()), b"x" * ln)
    assert len(arch.getvalue()) == exact
    assert zip_bound([]) == 22
    # AUTO never grows an entry; a forced deflated one is bounded by the raw stream's bound; an empty one is stored
    assert zip_bound([(b"a", 256, 5000, ZIP_AUTO)]) == 22 + 76 + 2 + 5000 == zip_bound([(b"a", 256, 5000)])
    assert zip_bound([(b"a", 256, 5000, ZIP_DEFLATED)]) == 22 + 76 + 2 + wrap_bound(5000, WRAP_RAW)
    assert zip_bound([(b"a", 0, 0, ZIP_DEFLATED)]) == 22 + 76 + 2
    for n in (1, 4096, 200000):
        data = os.urandom(n)
        assert len(zc.raw_deflate(data)) + 76 + 2 + 22 <= zip_bound([(b"a", 256, n, ZIP_DEFLATED)])
    # what the encoder refuses
    for bad in ([(b"a", 0, 1)], [(b"", 256, 1)], [(b"n" * 65536, 256, 1)], [(b"a", 256, -1)], [(b"a", 256, (1 << 31) - 1023)], [(b"a", 256, 1, 5)], [(b"a", 256, 1, -2)],
                [(b"a", 0, 0)] * 65536, [(b"a", 256, (1 << 31) - 1024, ZIP_STORED)] * 2):
        with pytest.raises(ValueError):
            zip_bound(bad)
    assert zip_bound([(b"a", 0, 0)] * 65535) == 22 + 78 * 65535
    assert zip_bound([(b"n" * 65535, 256, 1, ZIP_STORED)]) == 22 + 76 + 2 * 65535 + 1
    assert _native.lib().zs_zip_bound(None, 1) == -1 and _native.lib().zs_zip_bound(None, -1) == -1 and _native.lib().zs_zip_bound(None, 0) == 22


def test_device_calls_refuse_bad_arguments_before_any_device_work():
    """ZS_STREAM_ERROR without a context: no GPU is touched, nothing is read through the other pointers."""
    L = _native.lib()
    one = (ctypes.c_void_p * 1)(1)
    i64 = (ctypes.c_int64 * 1)(22)
    st = (ctypes.c_int * 1)(99)
    assert L.zs_zip_decode_files_batch(None, 1, one, i64, one, i64, i64, None, st, None) == -2
    assert L.zs_zip_decode_files_batch(None, -1, None, None, None, None, None, None, None, None) == -2
    puts = (_native.ZipPut * 1)()
    rows = (ctypes.POINTER(_native.ZipPut) * 1)(ctypes.cast(puts, ctypes.POINTER(_native.ZipPut)))
    cnt = (ctypes.c_int * 1)(1)
    assert L.zs_zip_encode_batch_device(None, 1, rows, cnt, one, i64, i64, st, 6, 0, 0, None) == -2
    assert st[0] == 99
