"""ZIP archives on the device, both directions (include/zsgpu.h zs_zip_*).  The yardstick is Python's zipfile and zlib: the
archives the decoder is given are built by tests/zip_cases.py and held against zipfile where they are built, the archives the
encoder writes are opened by zipfile.  Entry sizes are the smallest that reach each path: nothing, one byte, the one-wave
decoder below 1 KiB of compressed bytes, the block-parallel pass above, a Z_FIXED stream, stored blocks inside method 8, and
bytes that deflate does not shrink.  Outputs lie between guard bytes."""
import io
import os
import random
import zipfile
import zlib

import numpy as np
import pytest

import zip_cases as zc
from zlibstream_amd import (WRAP_RAW, ZIP_AUTO, ZIP_DEFLATED, ZIP_STORED, deflate_wrap_batch_device, wrap_bound, zip_bound, zip_decode_files_batch,
                            zip_encode_batch_device, zip_file_info)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL = 64, 0xEE
ZS_DATA_ERROR, ZS_BUF_ERROR = -3, -5
TEXT = open(os.path.join(ROOT, "tests", "golden", "corpus", "alice29.txt"), "rb").read()
_CACHE = {}


def shapes():
    """(name, plaintext, raw deflate body), made once."""
    if "shapes" not in _CACHE:
        rnd = random.Random(1)
        noise = bytes(rnd.randrange(256) for _ in range(4096))
        out = [("empty", b"", zc.raw_deflate(b"")), ("one", b"Z", zc.raw_deflate(b"Z")), ("text300", TEXT[:300], zc.raw_deflate(TEXT[:300])),
               ("text200k", (TEXT + TEXT)[:200000], zc.raw_deflate((TEXT + TEXT)[:200000])),
               ("fixed64k", TEXT[:65536], zc.raw_deflate(TEXT[:65536], 6, zlib.Z_FIXED)), ("stored100k", TEXT[:100000], zc.raw_deflate(TEXT[:100000], 0)),
               ("noise4k", noise, zc.raw_deflate(noise))]
        assert len(out[2][2]) < 1024 < len(out[3][2]) and len(out[6][2]) == 4096 + 5  # (deflate does not shrink the noise)
        _CACHE["shapes"] = out
    return _CACHE["shapes"]


def shape_entries(which=None):
    return [zc.entry(name.encode() + b".dat", plain, body=body) for name, plain, body in shapes() if which is None or name in which]


def run_decode(engine, files, caps=None):
    """zs_zip_decode_files_batch with every output between GUARD bytes of FILL.  caps: None for each file's total_len.  Returns
    (code, out_len[], entry codes[][], status[], out[i][:cap], files with a byte changed outside their capacity)."""
    import torch
    if caps is None:
        caps = [zip_file_info(f)[0]["total_len"] for f in files]
    out_off, off = [], GUARD
    for cap in caps:
        out_off.append(off)
        off = (off + cap + 255) // 256 * 256 + GUARD
    d_out = torch.full((off,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, lens, entry_codes, status = zip_decode_files_batch(engine, files, [d_out.data_ptr() + o for o in out_off], list(caps))
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    outside = got != FILL
    for o, cap in zip(out_off, caps):
        outside[o:o + cap] = False
    dirty = sorted({int(np.searchsorted(out_off, i, side="right")) - 1 for i in np.flatnonzero(outside)})
    return rc, lens, entry_codes, status, [got[o:o + cap].tobytes() for o, cap in zip(out_off, caps)], dirty


def check_decoded(files, entry_lists, rc, lens, entry_codes, status, outs, dirty):
    assert not dirty, dirty
    assert rc == 0 and list(status) == [0] * len(files)
    for f, ents, n, codes, out in zip(files, entry_lists, lens, entry_codes, outs):
        info, got = zip_file_info(f)
        assert n == info["total_len"] == sum(len(e["data"]) for e in ents) == len(out) and codes == [0] * len(ents)
        for g, e in zip(got, ents):
            assert out[g["out_off"]:g["out_off"] + g["len"]] == e["data"], e["name"]


def test_decode_one_archive_of_every_shape(engine):
    """Every shape deflated, and the empty and the noise entry stored as well, in one archive."""
    ents = shape_entries() + [zc.entry(b"stored/empty", b"", method=zc.STORED), zc.entry(b"stored/noise", shapes()[6][1], method=zc.STORED),
                              zc.entry(b"stored/text", TEXT[:70000], method=zc.STORED)]
    arch = zc.legal(zc.archive(ents), ents)
    check_decoded([arch], [ents], *run_decode(engine, [arch]))
    print("inf_wave_streams %d" % engine.counter("inf_wave_streams"))


def test_decode_three_archives_of_different_counts(engine):
    lists = [shape_entries(("text300",)), zc.three(), shape_entries() + zc.three(), []]
    files = [zc.legal(zc.archive(e, comment=b"archive %d" % k), e) for k, e in enumerate(lists)]
    check_decoded(files, lists, *run_decode(engine, files))


def test_decode_descriptor_zip64_and_prefixed_archives(engine):
    base = shape_entries(("one", "text300", "text200k", "noise4k"))
    dd = [zc.entry(e["name"], e["data"], body=e["body"], descriptor=True) for e in base] + [zc.entry(b"s", b"stored behind a descriptor", method=zc.STORED, descriptor=True)]
    z64 = [zc.entry(e["name"], e["data"], body=e["body"], local_extra=zc.zip64_extra(len(e["data"]), len(e["body"])),
                    lo=dict(version=45)) for e in base]  # (what force_zip64 writes: the field in the local header only)
    lists = [dd, z64, base, base, base]
    files = [zc.archive(dd), zc.archive(z64), zc.archive(base, end64=True), zc.archive(base, prefix=b"#!stub\n" * 3), zc.archive(base, prefix=b"12345", end64=True, comment=b"c")]
    for f, e in zip(files, lists):
        zc.legal(f, e)
    assert [zip_file_info(f)[0]["shift"] for f in files] == [0, 0, 0, 21, 5] and [zip_file_info(f)[0]["zip64"] for f in files] == [0, 0, 1, 0, 1]
    check_decoded(files, lists, *run_decode(engine, files))


def _stored_blocks(data):
    return zc.raw_deflate(data, 0)


MID = TEXT[1000:1300]
BAD_ENTRIES = {
    # name: (the middle entry, code, reason)
    "flipped body bit": (lambda: zc.entry(b"mid", MID, body=_stored_blocks(MID)[:40] + bytes([_stored_blocks(MID)[40] ^ 4]) + _stored_blocks(MID)[41:]), ZS_DATA_ERROR,
                         "incorrect data check"),
    "len one too small": (lambda: zc.entry(b"mid", MID, ce=dict(size=len(MID) - 1)), ZS_DATA_ERROR, "incorrect length check"),
    "len one too large": (lambda: zc.entry(b"mid", MID, ce=dict(size=len(MID) + 1)), ZS_DATA_ERROR, "incorrect length check"),
    "stored with a wrong CRC": (lambda: zc.entry(b"mid", MID, method=zc.STORED, ce=dict(crc=zlib.crc32(MID) ^ 1)), ZS_DATA_ERROR, "incorrect data check"),
    "method 12": (lambda: zc.entry(b"mid", MID, ce=dict(method=12), lo=dict(method=12)), ZS_DATA_ERROR, "unsupported compression method"),
    "encrypted": (lambda: zc.entry(b"mid", MID, flags=zc.ENCRYPTED), ZS_DATA_ERROR, "encrypted entries are not supported"),
    "local name differs": (lambda: dict(zc.entry(b"mid", MID), local_name=b"miD"), ZS_DATA_ERROR, "local header mismatch"),
    "comp_len past the file": (lambda: zc.entry(b"mid", MID, ce=dict(comp_len=1 << 20)), ZS_BUF_ERROR, "buffer error"),
}


@pytest.mark.parametrize("case", sorted(BAD_ENTRIES))
def test_decode_failing_entry_beside_whole_ones(engine, case):
    """The failing entry is the middle one of three, in the second of two files: its neighbours and the other file are
    byte-exact, the code and the message are the rule's."""
    make, code, reason = BAD_ENTRIES[case]
    first, last = zc.entry(b"first.txt", TEXT[:2000]), zc.entry(b"dir/last.bin", bytes(range(256)) * 2, method=zc.STORED)
    good_mid = zc.entry(b"mid", MID)
    good = zc.legal(zc.archive([first, good_mid, last]), [first, good_mid, last])
    mid = make()
    local_name = mid.pop("local_name", None)
    places = {}
    bad = zc.archive([first, mid, last], places=places)
    if local_name:
        at = places["local_off"][1] + 30
        bad = bad[:at] + local_name + bad[at + 3:]
    assert bad != good
    rc, lens, codes, status, outs, dirty = run_decode(engine, [good, bad])
    assert not dirty
    assert rc == code and list(status) == [0, code] and codes == [[0, 0, 0], [0, code, 0]]
    assert engine.last_error() == "file 1: entry 1: " + reason
    info, got = zip_file_info(bad)
    assert lens == [len(outs[0]), info["total_len"]]
    assert outs[0] == first["data"] + MID + last["data"]
    for k, e in ((0, first), (2, last)):
        assert outs[1][got[k]["out_off"]:got[k]["out_off"] + got[k]["len"]] == e["data"]


def test_decode_every_cut_of_an_archive_in_one_call(engine):
    ents = [zc.entry(b"a", TEXT[:150]), zc.entry(b"b", b"stored " * 9, method=zc.STORED), zc.entry(b"c", TEXT[150:260])]
    whole = zc.legal(zc.archive(ents), ents)
    assert 350 < len(whole) < 520
    files = [whole[:cut] for cut in range(len(whole) + 1)]
    total = sum(len(e["data"]) for e in ents)
    rc, lens, codes, status, outs, dirty = run_decode(engine, files, [total] * len(files))
    assert not dirty
    assert [k for k, s in enumerate(status) if s == 0] == [len(whole)] and rc == status[0] == ZS_BUF_ERROR
    assert set(status[:-1]) <= {ZS_DATA_ERROR, ZS_BUF_ERROR} and all(s == ZS_BUF_ERROR for s in status[:22])
    assert outs[-1] == b"".join(e["data"] for e in ents) and codes[-1] == [0, 0, 0]
    assert all(o == bytes([FILL]) * total for o in outs[:-1])  # (no directory, so nothing of them is decoded)
    assert engine.last_error().startswith("file 0: ")


def test_decode_short_out_cap(engine):
    lists = [shape_entries(("text300", "text200k")), zc.three()]
    files = [zc.archive(e) for e in lists]
    totals = [zip_file_info(f)[0]["total_len"] for f in files]
    rc, lens, codes, status, outs, dirty = run_decode(engine, files, [totals[0] - 1, totals[1]])
    assert not dirty
    assert rc == ZS_BUF_ERROR and list(status) == [ZS_BUF_ERROR, 0] and lens == totals and codes == [[], [0, 0, 0]]
    assert outs[0] == bytes([FILL]) * (totals[0] - 1) and outs[1] == b"".join(e["data"] for e in lists[1])
    assert engine.last_error() == "file 0: buffer error"
    check_decoded(files, lists, *run_decode(engine, files, totals))


# ---------------------------------------------------------------- encode
def run_encode(engine, archives, caps=None, shifts=None, level=6):
    """zs_zip_encode_batch_device: archives is a list of lists of (name, data[, method[, utf8[, date_time[, external_attr]]]])
    with data as bytes, which are put on the device at multiples of 256.  Every output lies at a multiple of 256 plus its shift,
    between GUARD bytes of FILL.  caps: None for zip_bound.  Returns (code, out_len[], status[], out[i][:cap], dirty, bounds)."""
    import torch
    blobs, off = [], 0
    for a in archives:
        for e in a:
            blobs.append((off, e[1]))
            off += (len(e[1]) + 255) // 256 * 256 + 256
    host = np.zeros(max(off, 256), dtype=np.uint8)
    for o, d in blobs:
        host[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    d_in = torch.from_numpy(host).cuda()
    at = iter(blobs)
    # (an empty entry's data pointer is null)
    puts = [[(e[0], d_in.data_ptr() + o if d else 0, len(d)) + tuple(e[2:]) for e, (o, d) in zip(a, at)] for a in archives]
    bounds = [zip_bound(p) for p in puts]
    caps = list(bounds) if caps is None else list(caps)
    shifts = [0] * len(archives) if shifts is None else shifts
    out_off, off = [], 0
    for cap, sh in zip(caps, shifts):
        off = (off + GUARD + 255) // 256 * 256 + sh
        out_off.append(off)
        off += cap
    d_out = torch.full((off + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 256 == 0
    torch.cuda.synchronize()
    rc, lens, status = zip_encode_batch_device(engine, puts, [d_out.data_ptr() + o for o in out_off], caps, level=level)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    outside = got != FILL
    for o, cap in zip(out_off, caps):
        outside[o:o + cap] = False
    dirty = sorted({int(np.searchsorted(out_off, i, side="right")) - 1 for i in np.flatnonzero(outside)})
    return rc, lens, status, [got[o:o + cap].tobytes() for o, cap in zip(out_off, caps)], dirty, bounds


def two_archives():
    a = [(name.encode() + b".dat", plain) for name, plain, _ in shapes()]
    b = [(b"forced/stored.txt", TEXT[:300], ZIP_STORED), (b"forced/deflated.bin", shapes()[6][1], ZIP_DEFLATED),
         ("grüße/text.txt".encode(), (TEXT + TEXT)[:200000], ZIP_AUTO, 1, (2024, 2, 29, 13, 14, 16), 0o100644 << 16), (b"forced/empty", b"", ZIP_DEFLATED)]
    return [a, b]


def raw_bodies(engine, datas, level):
    """deflate_wrap_batch_device(..., WRAP_RAW) of the same bytes: what a deflated entry's body has to be."""
    import torch
    outs = []
    for d in datas:
        src = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda()
        cap = wrap_bound(len(d), WRAP_RAW)
        dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        rc, lens, st = deflate_wrap_batch_device(engine, [src.data_ptr()], [len(d)], [dst.data_ptr()], [cap], WRAP_RAW, level=level)
        assert rc == 0
        outs.append(dst.cpu().numpy()[:lens[0]].tobytes())
    return outs


def check_archive(arch, entries, engine=None, level=None):
    """zipfile reads what was put; with an engine, every deflated body is the raw deflate call's."""
    with zipfile.ZipFile(io.BytesIO(arch)) as z:
        assert z.testzip() is None
        infos = z.infolist()
        assert len(infos) == len(entries) and not z.comment
        for i, e in zip(infos, entries):
            utf8 = len(e) > 3 and e[3]
            assert i.filename.encode("utf-8" if utf8 else "cp437") == e[0] and bool(i.flag_bits & 0x800) == bool(utf8) and z.read(i) == e[1]
            assert i.date_time == (e[4] if len(e) > 4 else (1980, 1, 1, 0, 0, 0)) and i.external_attr == (e[5] if len(e) > 5 else 0)
            assert i.create_system == (3 if i.external_attr >> 16 else 0) and i.extract_version == (20 if i.compress_type == 8 else 10) and not i.extra
            method = e[2] if len(e) > 2 else ZIP_AUTO
            if method != ZIP_AUTO or not e[1]:
                assert i.compress_type == (method if e[1] else 0)
            assert i.compress_type == 0 or i.compress_size < i.file_size or method == ZIP_DEFLATED
    info, got = zip_file_info(arch)
    assert info["comment_len"] == 0 and info["shift"] == 0 and info["cd_off"] + info["cd_len"] + 22 == len(arch) and all(g["status"] == 0 for g in got)
    if engine is not None:
        deflated = [(g, e) for g, e in zip(got, entries) if g["method"] == 8]
        for (g, e), want in zip(deflated, raw_bodies(engine, [e[1] for _, e in deflated], level)):
            assert arch[g["body_off"]:g["body_off"] + g["comp_len"]] == want, e[0]
            # AUTO would have kept the stored form had this not been shorter
            assert len(want) < len(e[1]) or (len(e) > 2 and e[2] == ZIP_DEFLATED)
    return got


@pytest.mark.parametrize("level", [1, 6, 9])
def test_encode_two_archives(engine, level):
    archives = two_archives()
    rc, lens, status, outs, dirty, bounds = run_encode(engine, archives, level=level)
    assert not dirty
    assert rc == 0 and list(status) == [0, 0] and all(n <= b for n, b in zip(lens, bounds))
    got = [check_archive(o[:n], a, engine, level) for o, n, a in zip(outs, lens, archives)]
    by_name = {g["name"]: g["method"] for g in got[0]}
    assert by_name["noise4k.dat"] == 0 and by_name["empty.dat"] == 0 and by_name["one.dat"] == 0  # (a 1-byte entry deflates to 3 bytes)
    assert [by_name[k + ".dat"] for k in ("text300", "text200k", "fixed64k", "stored100k")] == [8, 8, 8, 8]
    assert [g["method"] for g in got[1]] == [0, 8, 8, 0] and got[1][1]["comp_len"] > 4096
    assert all(o[n:] == bytes([FILL]) * (len(o) - n) for o, n in zip(outs, lens))
    if level == 6:
        _CACHE["encoded"] = [o[:n] for o, n in zip(outs, lens)]


def test_encode_out_cap_one_byte_short(engine):
    archives = two_archives()
    need = [len(a) for a in _CACHE["encoded"]] if "encoded" in _CACHE else run_encode(engine, archives)[1]
    for short in (0, 1):
        caps = [n - (k == short) for k, n in enumerate(need)]
        rc, lens, status, outs, dirty, _ = run_encode(engine, archives, caps=caps)
        assert not dirty
        assert rc == ZS_BUF_ERROR and list(status) == [ZS_BUF_ERROR if k == short else 0 for k in (0, 1)] and lens == need
        assert outs[short] == bytes([FILL]) * caps[short]
        check_archive(outs[1 - short], archives[1 - short])
        assert engine.last_error() == "buffer error"


def test_encode_at_odd_out_addresses(engine):
    one = [(b"a.txt", TEXT[:3000]), (b"b", b"x"), (b"noise", shapes()[6][1]), (b"c/d.txt", TEXT[3000:3300], ZIP_DEFLATED)]
    shifts = [0, 1, 7, 15]
    rc, lens, status, outs, dirty, _ = run_encode(engine, [one] * 4, shifts=shifts)
    assert not dirty
    assert rc == 0 and list(status) == [0] * 4 and len(set(lens)) == 1
    for o, n in zip(outs, lens):
        check_archive(o[:n], one)
    assert len({o[:n] for o, n in zip(outs, lens)}) == 1


def test_encode_empty_archive_and_refused_arguments(engine):
    rc, lens, status, outs, dirty, bounds = run_encode(engine, [[], [(b"only", b"")]])
    assert not dirty and rc == 0 and lens == [22, 22 + 76 + 8] == bounds
    check_archive(outs[0][:22], [])
    check_archive(outs[1][:lens[1]], [(b"only", b"")])
    import torch
    out = torch.full((1024,), FILL, dtype=torch.uint8, device="cuda")
    for bad in ([(b"", out.data_ptr(), 1)], [(b"a", 0, 1)], [(b"a", out.data_ptr(), 1, 3)], [(b"a", 0, 0)] * 65536):
        with pytest.raises(ValueError):
            zip_encode_batch_device(engine, [bad], [out.data_ptr()], [1024])
    torch.cuda.synchronize()
    assert bytes(out.cpu().numpy()) == bytes([FILL]) * 1024


def test_round_trip(engine):
    archives = two_archives()
    if "encoded" not in _CACHE:
        _, lens, _, outs, _, _ = run_encode(engine, archives)
        _CACHE["encoded"] = [o[:n] for o, n in zip(outs, lens)]
    encoded = _CACHE["encoded"]
    rc, lens, codes, status, outs, dirty = run_decode(engine, encoded)
    assert not dirty
    assert rc == 0 and list(status) == [0, 0] and codes == [[0] * len(a) for a in archives]
    assert outs == [b"".join(e[1] for e in a) for a in archives]
