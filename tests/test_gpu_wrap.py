"""Raw deflate and gzip on the batch calls, both directions, on the device (include/zsgpu.h ZS_WRAP_*).  The yardstick is
Python's zlib and gzip -- zlib.decompressobj(wbits=-15 | 31), its unused_data -- and, for the encoder's bytes, the oracle.
Stream sizes land on each inflate path: the one-wave decoder below 1 KiB of compressed bytes, the block-parallel pass above,
the fixed-block scan from 48 KiB of a Z_FIXED stream.  Outputs lie between guard bytes."""
import gzip
import os
import random
import struct
import zlib

import numpy as np
import pytest

import gzip_cases as gz
from zlibstream_amd import (WRAP_GZIP, WRAP_RAW, WRAP_ZLIB, deflate_wrap_batch_device, gzip_decode_files_batch, inflate_wrap_batch_device,
                            wrap_bound)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL = 64, 0xEE
ZS_STREAM_END, ZS_DATA_ERROR, ZS_BUF_ERROR = 1, -3, -5
TEXT = open(os.path.join(ROOT, "tests", "golden", "corpus", "alice29.txt"), "rb").read()
_CACHE = {}


def bodies():
    """(name, plaintext, raw deflate stream), made once."""
    if "bodies" not in _CACHE:
        out = []
        for level in (1, 6, 9):
            out.append(("text300_L%d" % level, TEXT[:300], gz.raw_deflate(TEXT[:300], level)))
            out.append(("text200k_L%d" % level, (TEXT + TEXT)[:200000], gz.raw_deflate((TEXT + TEXT)[:200000], level)))
        out.append(("fixed64k", TEXT[:65536], gz.raw_deflate(TEXT[:65536], 6, zlib.Z_FIXED)))
        out.append(("fixed150k_L1", TEXT[:150000], gz.raw_deflate(TEXT[:150000], 1, zlib.Z_FIXED)))  # compressed: above 48 KiB
        out.append(("stored100k", TEXT[:100000], gz.raw_deflate(TEXT[:100000], 0)))
        out.append(("empty", b"", gz.raw_deflate(b"")))
        # one fixed block of n 9-bit literals and the end-of-block code: 3 + 9 n + 7 bits -- 64 for six of them, 19 for one
        whole = bytes([150, 160, 170, 180, 190, 200])
        out.append(("ends_on_a_byte", whole, gz.raw_deflate(whole, 6, zlib.Z_FIXED)))
        out.append(("ends_mid_byte", whole[:1], gz.raw_deflate(whole[:1], 6, zlib.Z_FIXED)))
        assert len(out[-2][2]) == 8 and len(out[-1][2]) == 3
        assert len(out[0][2]) < 1024 < len(out[1][2]) and len(out[7][2]) >= 48 * 1024
        _CACHE["bodies"] = out
    return _CACHE["bodies"]


def run_inflate(engine, streams, caps, wrap, in_shift=0):
    """zs_inflate_wrap_batch_device on device buffers: every input at a multiple of 256 plus in_shift, every output between
    GUARD bytes of FILL, the ones behind it beginning at out + cap.  Returns (code, out_len[], in_used[], status[], out[i][:cap],
    streams with a byte changed outside every capacity)."""
    import torch
    in_off, off = [], 0
    for z in streams:
        in_off.append(off + in_shift)
        off += (len(z) + in_shift + 255) // 256 * 256 + 256
    host_in = np.zeros(off, dtype=np.uint8)
    for o, z in zip(in_off, streams):
        host_in[o:o + len(z)] = np.frombuffer(z, dtype=np.uint8)
    out_off, off = [], GUARD
    for cap in caps:
        out_off.append(off)
        off = (off + cap + 255) // 256 * 256 + GUARD
    d_in = torch.from_numpy(host_in).cuda()
    d_out = torch.full((off,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, lens, used, status = inflate_wrap_batch_device(engine, [d_in.data_ptr() + o for o in in_off], [len(z) for z in streams],
                                                       [d_out.data_ptr() + o for o in out_off], list(caps), wrap)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    outside = got != FILL
    for o, cap in zip(out_off, caps):
        outside[o:o + cap] = False
    dirty = sorted({int(np.searchsorted(out_off, i, side="right")) - 1 for i in np.flatnonzero(outside)})
    return rc, lens, used, status, [got[o:o + cap].tobytes() for o, cap in zip(out_off, caps)], dirty


def zlib_says(z, wbits):
    d = zlib.decompressobj(wbits)
    out = d.decompress(z)
    assert d.eof
    return out, len(z) - len(d.unused_data)


def check_whole(names, streams, plains, wbits, rc, lens, used, status, outs, dirty):
    assert not dirty, [names[i] for i in dirty]
    bad = []
    for k, (name, z, plain) in enumerate(zip(names, streams, plains)):
        want, want_used = zlib_says(z, wbits)
        assert want == plain
        if (status[k], lens[k], used[k], outs[k][:lens[k]]) != (ZS_STREAM_END, len(plain), want_used, plain):
            bad.append((name, status[k], lens[k], len(plain), used[k], want_used))
    assert not bad, bad
    assert rc == 0


@pytest.mark.parametrize("wrap", [WRAP_RAW, WRAP_GZIP])
def test_inflate_one_batch(engine, wrap):
    """Every body with nothing and with 7 bytes of garbage behind it, in one batch: bytes and in_used against zlib."""
    names, streams, plains = [], [], []
    for name, plain, body in bodies():
        z = body if wrap == WRAP_RAW else gz.header() + body + gz.trailer(plain)
        for tail in (b"", b"\x9dgarbage"[:7]):
            names.append(name + ("+7" if tail else "")), streams.append(z + tail), plains.append(plain)
    res = run_inflate(engine, streams, [len(p) for p in plains], wrap)
    print("inf_wave_streams %d of %d" % (engine.counter("inf_wave_streams"), len(streams)))
    check_whole(names, streams, plains, -15 if wrap == WRAP_RAW else 31, *res)


@pytest.mark.parametrize("shift", [0, 3])
def test_gzip_bodies_at_odd_offsets(engine, shift):
    """The bodies behind headers of 10, 11, 12, 13 and 16 bytes (no name; a name of 0, 1, 2 and 5 bytes): every alignment
    class mod 4, off the 16-byte grid and on it; and the same with the members themselves 3 bytes off their 256-byte places."""
    names, streams, plains = [], [], []
    for nm in (None, b"", b"a", b"ab", b"abcde"):
        for name, plain, body in bodies():
            hd = gz.header() if nm is None else gz.header(gz.FNAME, name=nm)
            names.append("%s behind %d" % (name, len(hd))), streams.append(hd + body + gz.trailer(plain)), plains.append(plain)
    assert {len(gz.header(gz.FNAME, name=nm)) for nm in (b"", b"a", b"ab", b"abcde")} | {len(gz.header())} == {10, 11, 12, 13, 16}
    res = run_inflate(engine, streams, [len(p) for p in plains], WRAP_GZIP, in_shift=shift)
    check_whole(names, streams, plains, 31, *res)


def test_gzip_header_fields_on_the_device(engine):
    """FEXTRA (a BGZF subfield among others), FNAME, FCOMMENT and a right FHCRC in front of a body of each path."""
    extra = b"RA\x03\x00abc" + struct.pack("<BBHH", 66, 67, 2, 999)
    hd = gz.header(gz.FEXTRA | gz.FNAME | gz.FCOMMENT | gz.FHCRC | gz.FTEXT, extra=extra, name=b"n" * 300, comment=b"said", mtime=77, xfl=2, os_=3)
    names, streams, plains = [], [], []
    for name, plain, body in bodies():
        names.append(name), streams.append(hd + body + gz.trailer(plain)), plains.append(plain)
    res = run_inflate(engine, streams, [len(p) for p in plains], WRAP_GZIP)
    check_whole(names, streams, plains, 31, *res)


def member_400():
    for n in range(300, 900):
        m = gz.member(TEXT[1000:1000 + n], flg=gz.FEXTRA | gz.FNAME | gz.FCOMMENT | gz.FHCRC, extra=b"ab\x02\x00xy", name=b"name", comment=b"c")
        if len(m) == 400:
            return TEXT[1000:1000 + n], m
    raise AssertionError("no 400-byte member")


@pytest.mark.parametrize("what,at,message", [("crc", -8, "incorrect data check"), ("crc", -5, "incorrect data check"),
                                             ("isize", -4, "incorrect length check"), ("isize", -1, "incorrect length check"),
                                             ("fhcrc", None, "header crc mismatch"), ("flags", 3, "unknown header flags set"),
                                             ("method", 2, "unknown compression method"), ("magic", 1, "incorrect header check")])
@pytest.mark.parametrize("big", [False, True])
def test_gzip_errors_beside_the_legal_member(engine, what, at, message, big):
    """A member of each error class between two copies of its legal self (one-wave decoder: 400 bytes; block-parallel pass:
    200 KB of text), status and message; a trailer's error leaves the whole output, a header's none."""
    if big:
        plain = (TEXT + TEXT)[:200000]
        good = gz.member(plain, flg=gz.FNAME | gz.FHCRC, name=b"name")
        head = len(gz.header(gz.FNAME | gz.FHCRC, name=b"name"))
    else:
        plain, good = member_400()
        head = len(gz.header(gz.FEXTRA | gz.FNAME | gz.FCOMMENT | gz.FHCRC, extra=b"ab\x02\x00xy", name=b"name", comment=b"c"))
    bad = bytearray(good)
    if what == "fhcrc":
        bad[head - 1] ^= 0x10
    elif what == "flags":
        bad[3] |= 0x40
    elif what == "method":
        bad[2] = 7
    else:
        bad[at] ^= 0x01
    with pytest.raises(zlib.error, match=message):
        zlib.decompressobj(31).decompress(bytes(bad))  # (zlib's text for it)
    rc, lens, used, status, outs, dirty = run_inflate(engine, [good, bytes(bad), good], [len(plain)] * 3, WRAP_GZIP)
    assert not dirty
    assert status == [ZS_STREAM_END, ZS_DATA_ERROR, ZS_STREAM_END] and rc == ZS_DATA_ERROR
    assert engine.last_error() == message
    assert used == [len(good), 0, len(good)]
    assert lens == [len(plain), len(plain) if what in ("crc", "isize") else 0, len(plain)]
    assert outs[0] == plain and outs[2] == plain and outs[1][:lens[1]] == plain[:lens[1]]


def test_gzip_every_cut_of_a_400_byte_member(engine):
    """Header, body and trailer cut at every byte, beside the whole member: a buffer error, a prefix, nothing outside."""
    plain, m = member_400()
    cuts = [m[:n] for n in range(len(m))]
    rc, lens, used, status, outs, dirty = run_inflate(engine, [m] + cuts + [m], [len(plain)] * (len(cuts) + 2), WRAP_GZIP)
    assert not dirty
    assert status[0] == status[-1] == ZS_STREAM_END and outs[0] == outs[-1] == plain and used[0] == used[-1] == 400
    assert [n for n in range(len(cuts)) if status[1 + n] != ZS_BUF_ERROR] == []
    assert [n for n in range(len(cuts)) if used[1 + n] != 0 or lens[1 + n] > len(plain) or outs[1 + n][:lens[1 + n]] != plain[:lens[1 + n]]] == []
    assert rc == ZS_BUF_ERROR and engine.last_error() == "buffer error"
    assert lens[1 + 399] == len(plain) and lens[1 + 10] == 0  # inside the trailer: the whole output; inside the header: none


def test_raw_cuts_and_short_capacities(engine):
    """A raw stream cut at every byte, and whole into capacities one byte short: buffer errors and prefixes."""
    plain = TEXT[2000:2600]
    z = gz.raw_deflate(plain, 6)
    cuts = [z[:n] for n in range(len(z))]
    rc, lens, used, status, outs, dirty = run_inflate(engine, cuts + [z, z], [len(plain)] * (len(cuts) + 1) + [len(plain) - 1], WRAP_RAW)
    assert not dirty
    assert status == [ZS_BUF_ERROR] * len(cuts) + [ZS_STREAM_END, ZS_BUF_ERROR] and rc == ZS_BUF_ERROR
    assert used[:len(cuts)] == [0] * len(cuts) and used[-2:] == [len(z), 0]
    assert [n for n in range(len(outs)) if outs[n][:lens[n]] != plain[:lens[n]]] == [] and outs[-2] == plain


def test_wrap_zlib_is_the_zlib_call(engine):
    """ZS_WRAP_ZLIB against zs_inflate_batch_device on one batch with good, corrupt and truncated streams of both paths."""
    import ctypes
    streams, caps = [], []
    for plain in (TEXT[:300], (TEXT + TEXT)[:200000], b""):
        z = zlib.compress(plain, 6)
        broken = bytearray(z)
        broken[-1] ^= 1
        streams += [z, bytes(broken), z[:len(z) - 2], z + b"tail"]
        caps += [len(plain)] * 4
    streams.append(zlib.compress(TEXT[:5000])), caps.append(4999)
    a = run_inflate(engine, streams, caps, WRAP_ZLIB)
    said = engine.last_error()
    import torch
    d_in = [torch.from_numpy(np.frombuffer(z, dtype=np.uint8).copy()).cuda() for z in streams]
    d_out = [torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda") for cap in caps]
    rc, lens, status = engine._call_inflate(engine._lib.zs_inflate_batch_device, [t.data_ptr() for t in d_in], [len(z) for z in streams],
                                            [t.data_ptr() for t in d_out], caps, (ctypes.c_void_p(0),))
    assert (a[0], a[1], a[3]) == (rc, lens, status) and said == engine.last_error()
    assert [a[4][k][:lens[k]] for k in range(len(streams))] == [d_out[k].cpu().numpy().tobytes()[:lens[k]] for k in range(len(streams))]
    want_used = [len(z) if st == ZS_STREAM_END else 0 for z, st in zip(streams, status)]
    for k in (3, 7, 11):
        want_used[k] -= 4  # ("tail" is not the stream's)
    assert a[2] == want_used and status[0] == status[3] == ZS_STREAM_END and status[1] == ZS_DATA_ERROR and status[2] == ZS_BUF_ERROR


# ------------------------------------------------------------------ deflate
SIZES = (0, 1, 300, 65537, 1 << 20)


def deflate_inputs():
    if "inputs" not in _CACHE:
        corpus = b"".join(open(os.path.join(ROOT, "tests", "golden", "corpus", f), "rb").read() for f in ("alice29.txt", "fields.c", "kennedy.xls"))
        _CACHE["inputs"] = [corpus[5000:5000 + n] for n in SIZES]
    return _CACHE["inputs"]


def run_deflate(engine, datas, caps, wrap, level, strategy):
    import torch
    in_off, off = [], 0
    for d in datas:
        in_off.append(off)
        off += (len(d) + 255) // 256 * 256 + 256
    host_in = np.zeros(off, dtype=np.uint8)
    for o, d in zip(in_off, datas):
        host_in[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    out_off, off = [], GUARD
    for k, cap in enumerate(caps):
        out_off.append(off + (k % 3))  # (destinations of every alignment)
        off = (off + 3 + cap + 255) // 256 * 256 + GUARD
    d_in = torch.from_numpy(host_in).cuda()
    d_out = torch.full((off,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, lens, status = deflate_wrap_batch_device(engine, [d_in.data_ptr() + o for o in in_off], [len(d) for d in datas],
                                                 [d_out.data_ptr() + o for o in out_off], list(caps), wrap, level, strategy)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    outside = got != FILL
    for o, cap in zip(out_off, caps):
        outside[o:o + cap] = False
    return rc, lens, status, [got[o:o + cap].tobytes() for o, cap in zip(out_off, caps)], bool(outside.any())


def framed(z, data, wrap, level):
    if wrap == WRAP_RAW:
        return z[2:-4]
    return struct.pack("<BBBBIBB", 0x1F, 0x8B, 8, 0, 0, 2 if level == 9 else 4 if level == 1 else 0, 255) + z[2:-4] + struct.pack("<II", zlib.crc32(data), len(data))


@pytest.mark.parametrize("strategy", [0, 3])
@pytest.mark.parametrize("level", [1, 6, 9])
def test_deflate_into_raw_and_gzip(engine, oracle, level, strategy):
    datas = deflate_inputs()
    zs = [oracle.compress(d, level, strategy) for d in datas]
    for wrap in (WRAP_RAW, WRAP_GZIP):
        caps = [wrap_bound(len(d), wrap) for d in datas]
        rc, lens, status, outs, dirty = run_deflate(engine, datas, caps, wrap, level, strategy)
        assert rc == 0 and status == [0] * len(datas) and not dirty
        for d, z, n, out in zip(datas, zs, lens, outs):
            assert out[:n] == framed(z, d, wrap, level), (len(d), wrap)
            if wrap == WRAP_GZIP:
                assert gzip.decompress(out[:n]) == d
            else:
                assert zlib.decompressobj(-15).decompress(out[:n]) == d
    # ZS_WRAP_ZLIB is the zlib call
    rc, lens, status, outs, dirty = run_deflate(engine, datas, [wrap_bound(len(d), WRAP_ZLIB) for d in datas], WRAP_ZLIB, level, strategy)
    assert rc == 0 and [out[:n] for out, n in zip(outs, lens)] == zs and not dirty


@pytest.mark.parametrize("wrap", [WRAP_RAW, WRAP_GZIP])
def test_deflate_capacity_one_byte_short(engine, oracle, wrap):
    datas = [TEXT[:70000], TEXT[100:40100], TEXT[:300], b""]
    want = [framed(oracle.compress(d, 6, 0), d, wrap, 6) for d in datas]
    for short in range(len(datas)):
        caps = [len(w) - (1 if k == short else 0) for k, w in enumerate(want)]
        rc, lens, status, outs, dirty = run_deflate(engine, datas, caps, wrap, 6, 0)
        assert not dirty
        assert rc == ZS_BUF_ERROR and status == [ZS_BUF_ERROR if k == short else 0 for k in range(len(datas))]
        assert engine.last_error() == "buffer error"
        assert lens == [len(w) for w in want]  # (the short one's: what it needs)
        for k in range(len(datas)):
            if k != short:
                assert outs[k] == want[k]
            else:
                assert outs[k] == bytes([FILL]) * caps[k]  # nothing is written for it


# ------------------------------------------------------------------ files
def run_files(engine, files, caps):
    import torch
    out_off, off = [], GUARD
    for cap in caps:
        out_off.append(off)
        off = (off + cap + 255) // 256 * 256 + GUARD
    d_out = torch.full((off,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    status, lens, members = gzip_decode_files_batch(engine, files, [d_out.data_ptr() + o for o in out_off], caps)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    outside = got != FILL
    for o, cap in zip(out_off, caps):
        outside[o:o + cap] = False
    return status, lens, members, [got[o:o + cap].tobytes() for o, cap in zip(out_off, caps)], bool(outside.any())


def file_set():
    if "files" not in _CACHE:
        rnd = random.Random(11)
        src = TEXT + TEXT
        blocks = []
        for k in range(40):
            n = (100, 61440)[k] if k < 2 else rnd.randrange(100, 61441)
            at = rnd.randrange(0, len(src) - n)
            blocks.append(src[at:at + n])
        parts = [TEXT[:50000], b"", TEXT[50000:50300]]
        plain3 = gz.member(parts[0], flg=gz.FNAME, name=b"a.txt") + gz.member(parts[1]) + gz.member(parts[2], body=gz.raw_deflate(parts[2], 9))
        padded = gz.member(TEXT[:3000]) + b"\0" * 5
        _CACHE["files"] = (blocks, gz.bgzf_file(blocks), plain3, padded)
    return _CACHE["files"]


def test_files_bgzf_beside_plain_and_padded(engine):
    blocks, bgzf, plain3, padded = file_set()
    files = [bgzf, plain3, padded]
    want = [gzip.decompress(f) for f in files]
    assert want[0] == b"".join(blocks)
    status, lens, members, outs, dirty = run_files(engine, files, [len(w) for w in want])
    assert not dirty and status == [0, 0, 0], engine.last_error()
    assert members == [41, 3, 1] and lens == [len(w) for w in want]
    assert outs == want


def test_files_fail_for_themselves(engine):
    """A BGZF block with a wrong ISIZE (one more, one less), bytes that are no member behind a plain file's second member, a
    plain file cut inside its third member: each beside files that are whole."""
    blocks, bgzf, plain3, padded = file_set()
    sizes = [len(gz.bgzf_block(b)) for b in blocks]
    at7 = sum(sizes[:8]) - 4  # block 7's ISIZE
    files, want_st, want_len, want_n, says = [bgzf], [0], [sum(map(len, blocks))], [41], []
    for delta in (1, -1):
        b = bytearray(bgzf)
        struct.pack_into("<I", b, at7, len(blocks[7]) + delta)
        files.append(bytes(b)), want_st.append(ZS_DATA_ERROR), want_len.append(sum(map(len, blocks[:7]))), want_n.append(7)
    two = len(plain3) - len(gz.member(TEXT[50000:50300], body=gz.raw_deflate(TEXT[50000:50300], 9)))
    files.append(plain3[:two] + b"\0\0junk"), want_st.append(ZS_DATA_ERROR), want_len.append(50000), want_n.append(2)
    files.append(plain3[:-3]), want_st.append(ZS_BUF_ERROR), want_len.append(50000), want_n.append(2)
    files.append(padded), want_st.append(0), want_len.append(3000), want_n.append(1)
    whole = b"".join(blocks)
    status, lens, members, outs, dirty = run_files(engine, files, [len(whole) + 8, len(whole) + 8, len(whole) + 8, 50300, 50300, 3000])
    assert not dirty
    assert status == want_st and members == want_n and lens == want_len
    assert engine.last_error() == "file 1: incorrect length check"
    assert outs[0][:lens[0]] == whole and outs[5] == TEXT[:3000]
    for k in (1, 2):
        assert outs[k][:lens[k]] == whole[:lens[k]]
    for k in (3, 4):
        assert outs[k][:lens[k]] == TEXT[:50000]
    # each failing file alone, for its message
    for k, text in ((1, "incorrect length check"), (2, "incorrect length check"), (3, "incorrect header check"), (4, "buffer error")):
        st, _, _, _, _ = run_files(engine, [files[k]], [len(whole) + 8])
        assert st == [want_st[k]] and engine.last_error() == "file 0: " + text
