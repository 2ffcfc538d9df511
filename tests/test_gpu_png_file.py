"""Whole PNG files on the device: pixels to files (zs_png_encode_batch_device) and files to pixels (zs_png_decode_files_batch).
The references are Python's struct, zlib.crc32 and zlib.decompress and a numpy restatement of PNG specification 9.2 (and 8.2 for
the interlaced inputs); every comparison is exact.  Pillow, where installed, opens what the encoder writes and writes what the
decoder reads, in test functions of their own."""
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZS_OK, ZS_STREAM_ERROR, ZS_DATA_ERROR, ZS_BUF_ERROR = 0, -2, -3, -5
SIG = b"\x89PNG\r\n\x1a\n"
SHAPES = ((1, 1), (3, 5), (33, 31), (65, 129), (1000, 3))
# PNG specification table 11.1
LEGAL = [(c, d) for c, ds in ((0, (1, 2, 4, 8, 16)), (2, (8, 16)), (3, (1, 2, 4, 8)), (4, (8, 16)), (6, (8, 16))) for d in ds]
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))  # xstart, ystart, xstep, ystep
GUARD = 64


# ---------------------------------------------------------------- the specification, restated
def _row_bytes(w, bits):
    return (w * bits + 7) // 8


def _random_rows(rng, w, h, bits):
    """(h, row_bytes) raw scanlines of random pixels, padding bits zero"""
    rows = rng.integers(0, 256, (h, _row_bytes(w, bits)), dtype=np.uint8)
    used = (w * bits) % 8
    if used:
        rows[:, -1] &= (0xFF00 >> used) & 0xFF
    return rows


def _smooth_rows(w, h, bits):
    y, x = np.mgrid[0:h, 0:_row_bytes(w, bits)]
    rows = ((x // max(1, bits // 8)) * 3 + y * 5 + (x % max(1, bits // 8)) * 40).astype(np.uint8)
    used = (w * bits) % 8
    if used:
        rows[:, -1] &= (0xFF00 >> used) & 0xFF
    return rows


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _filter_rows(rows, bpp, types):
    """PNG specification 9.2, forward: (h, rb) raw scanlines -> (h, 1 + rb) filtered ones with the given type per row"""
    x = rows.astype(np.int32)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp] if x.shape[1] > bpp else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, bpp:] = b[:, :-bpp] if x.shape[1] > bpp else 0
    pred = np.stack([np.zeros_like(x), a, b, (a + b) >> 1, _paeth(a, b, c)])
    t = np.asarray(types, dtype=np.int64)
    f = (x - pred[t, np.arange(x.shape[0])]) & 255
    return np.concatenate([t[:, None].astype(np.uint8), f.astype(np.uint8)], axis=1)


def _unfilter(payload, rb, h, bpp):
    """PNG specification 9.2, inverse: the inflated IDAT payload of a non-interlaced image -> (h, rb) raw scanlines"""
    assert len(payload) == h * (rb + 1)
    out = bytearray(h * rb)
    prev = bytearray(rb)
    for y in range(h):
        t, x = payload[y * (rb + 1)], payload[y * (rb + 1) + 1:(y + 1) * (rb + 1)]
        assert t <= 4
        if t == 0:
            row = bytearray(x)
        elif t == 2:
            row = bytearray((np.frombuffer(x, dtype=np.uint8) + np.frombuffer(bytes(prev), dtype=np.uint8)).tobytes())  # (uint8 wraps)
        else:
            row = bytearray(rb)  # Sub, Average and Paeth read the row's own earlier bytes: a byte at a time
            for i in range(rb):
                a, c = (row[i - bpp], prev[i - bpp]) if i >= bpp else (0, 0)
                b = prev[i]
                if t == 1:
                    pr = a
                elif t == 3:
                    pr = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pr = a if pa <= pb and pa <= pc else b if pb <= pc else c
                row[i] = (x[i] + pr) & 255
        out[y * rb:(y + 1) * rb] = prev = row
    return np.frombuffer(bytes(out), dtype=np.uint8).reshape(h, rb)


def _unpack(rows, w, bits):
    if bits >= 8:
        return rows.reshape(rows.shape[0], w, bits // 8)
    b = np.unpackbits(rows, axis=1)[:, :w * bits].reshape(rows.shape[0], w, bits)
    return (b * (1 << np.arange(bits - 1, -1, -1))).sum(axis=2).astype(np.uint8)


def _pack(px, bits):
    if bits >= 8:
        return np.ascontiguousarray(px).reshape(px.shape[0], -1)
    b = (px[:, :, None] >> np.arange(bits - 1, -1, -1)) & 1
    return np.packbits(b.reshape(px.shape[0], -1).astype(np.uint8), axis=1)


def _payload(rng, rows, w, bits, interlace):
    """the IDAT payload before compression, random filter types per row (per pass row; PNG specification 8.2 by slices)"""
    bpp = max(1, bits // 8)
    if not interlace:
        return _filter_rows(rows, bpp, rng.integers(0, 5, rows.shape[0])).tobytes()
    px = _unpack(rows, w, bits)
    out = b""
    for xs, ys, xst, yst in ADAM7:
        sub = px[ys::yst, xs::xst]
        if sub.shape[0] and sub.shape[1]:
            out += _filter_rows(_pack(sub, bits), bpp, rng.integers(0, 5, sub.shape[0])).tobytes()
    return out


def chunk(ctype, data, crc=None):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data) if crc is None else crc)


def build_png(w, h, depth, color, interlace, stream, cuts=(), before=(), after=()):
    """a file around `stream`, its IDAT chunks ending at the given cumulative cuts (and at the stream's end)"""
    parts, at = [], 0
    for e in list(cuts) + [len(stream)]:
        e = max(at, min(e, len(stream)))
        parts.append(stream[at:e])
        at = e
    return (SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color, 0, 0, interlace)) + b"".join(before) +
            b"".join(chunk(b"IDAT", p) for p in parts) + b"".join(after) + chunk(b"IEND", b""))


def parse_png(f):
    """-> list of (type, data, stored crc, offset) by struct alone; asserts the signature and that the chunks tile the file"""
    assert f[:8] == SIG
    out, at = [], 8
    while at < len(f):
        n, t = struct.unpack(">I4s", f[at:at + 8])
        assert at + 12 + n <= len(f), (at, n, len(f))
        out.append((t, f[at + 8:at + 8 + n], struct.unpack(">I", f[at + 8 + n:at + 12 + n])[0], at))
        at += 12 + n
    assert at == len(f)
    return out


# ---------------------------------------------------------------- device plumbing
def _cuda(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def _encode(engine, rows_list, dims, filters, level, chunk_bytes=0, extra=None, caps=None, rows_per_write=1, offsets=None, stream=None):
    """-> (rc, lengths, statuses, [the bytes of every output buffer, guard included], offsets); every output sits at its own
    byte offset inside a 0xEE-filled tensor with GUARD bytes behind its capacity"""
    import torch
    from zlibstream_amd import deflate_bound, png_encode_batch_device, png_file_bound
    n = len(rows_list)
    d_px = [_cuda(r.tobytes()) for r in rows_list]
    if caps is None:
        caps = [png_file_bound(deflate_bound(r.shape[0] * (r.shape[1] + 1)), chunk_bytes, len(extra[i]) if extra else 0) for i, r in enumerate(rows_list)]
    offsets = offsets or [(5 * i + 3) % 16 for i in range(n)]
    d_out = [torch.full((o + c + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for o, c in zip(offsets, caps)]
    torch.cuda.synchronize()  # torch filled them on its own stream; the engine's stream does not wait for that one
    rc, lens, st = png_encode_batch_device(engine, [t.data_ptr() for t in d_px], [d[0] for d in dims], [d[1] for d in dims], [d[2] for d in dims],
                                           [d[3] for d in dims], filters, [t.data_ptr() + o for t, o in zip(d_out, offsets)], caps, extra=extra,
                                           rows_per_write=rows_per_write, idat_chunk_bytes=chunk_bytes, level=level, stream=stream, return_status=True)
    return rc, lens, st, [t.cpu().numpy().tobytes() for t in d_out], offsets, caps


def _idat_reference(engine, rows_list, dims, filters, level, rows_per_write=1):
    """what png_idat_batch_device returns for the same arguments"""
    import torch
    from zlibstream_amd import deflate_bound, png_idat_batch_device
    d_px = [_cuda(r.tobytes()) for r in rows_list]
    caps = [deflate_bound(r.shape[0] * (r.shape[1] + 1)) for r in rows_list]
    d_z = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    torch.cuda.synchronize()
    lens = png_idat_batch_device(engine, [t.data_ptr() for t in d_px], [r.shape[1] for r in rows_list], [r.shape[0] for r in rows_list],
                                 [max(1, d[2] * CHANNELS[d[3]] // 8) for d in dims], filters, [t.data_ptr() for t in d_z], caps,
                                 rows_per_write=rows_per_write, level=level)
    return [t[:k].cpu().numpy().tobytes() for t, k in zip(d_z, lens)]


def _check_file(buf, off, cap, length, dims, rows, want_stream, extra=b"", chunk_bytes=0):
    """every property of one encoded file; returns its chunks"""
    w, h, depth, color = dims
    assert buf[:off] == b"\xEE" * off and buf[off + length:] == b"\xEE" * (len(buf) - off - length), "bytes outside the file were written"
    f = buf[off:off + length]
    chunks = parse_png(f)
    for t, data, crc, at in chunks:
        assert crc == zlib.crc32(t + data), (t, at)
    assert chunks[0][0] == b"IHDR" and chunks[0][1] == struct.pack(">IIBBBBB", w, h, depth, color, 0, 0, 0)
    assert chunks[-1][0] == b"IEND" and chunks[-1][1] == b""
    first = next(i for i, c in enumerate(chunks) if c[0] == b"IDAT")
    assert f[33:chunks[first][3]] == extra, "the caller's chunks are not verbatim between IHDR and IDAT"
    idat = [c for c in chunks[first:-1]]
    assert all(c[0] == b"IDAT" for c in idat)
    stream = b"".join(c[1] for c in idat)
    assert stream == want_stream, "the IDAT data is not png_idat_batch_device's stream"
    if chunk_bytes:
        assert [len(c[1]) for c in idat] == [min(chunk_bytes, len(stream) - a) for a in range(0, len(stream), chunk_bytes)]
    else:
        assert len(idat) == 1
    bits = depth * CHANNELS[color]
    got = _unfilter(zlib.decompress(stream), _row_bytes(w, bits), h, max(1, bits // 8))
    assert got.tobytes() == rows.tobytes(), "the file does not hold the pixels"
    return chunks


def _decode_files(engine, files, caps=None, stream=None):
    """-> (statuses, infos, one uint8 array per file); every output inside a 0xEE-filled tensor of its own"""
    import torch
    from zlibstream_amd import png_decode_files_batch, png_file_info
    sizes = []
    for f in files:
        try:
            sizes.append(png_file_info(f)["pixel_bytes"])
        except Exception:
            sizes.append(1 << 16)  # (a broken file: room for whatever its IHDR may say at the shapes used here)
    caps = caps or sizes
    d_out = [torch.full((max(c, 1) + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for c in caps]
    torch.cuda.synchronize()
    st, infos = png_decode_files_batch(engine, files, [t.data_ptr() for t in d_out], caps, stream=stream)
    return st, infos, [t.cpu().numpy() for t in d_out]


# ---------------------------------------------------------------- encode
@pytest.fixture(scope="module")
def images():
    """(color, depth) -> the raw scanlines of SHAPES, made once"""
    rng = np.random.default_rng(7301)
    return {(c, d): [_smooth_rows(w, h, d * CHANNELS[c]) if (w + h) % 2 else _random_rows(rng, w, h, d * CHANNELS[c]) for w, h in SHAPES] for c, d in LEGAL}


@pytest.mark.parametrize("level", [1, 6])
@pytest.mark.parametrize("color,depth", LEGAL)
def test_encode_every_legal_pair_and_filter(engine, images, color, depth, level):
    rows_list = [r for r in images[color, depth] for _ in range(6)]
    dims = [(w, h, depth, color) for w, h in SHAPES for _ in range(6)]
    filters = [f for _ in SHAPES for f in range(6)]
    want = _idat_reference(engine, rows_list, dims, filters, level)
    rc, lens, st, bufs, offs, caps = _encode(engine, rows_list, dims, filters, level)
    assert rc == ZS_OK and st == [ZS_OK] * len(dims), engine.last_error()
    for i in range(len(dims)):
        _check_file(bufs[i], offs[i], caps[i], lens[i], dims[i], rows_list[i], want[i])


def test_encode_idat_chunk_sizes(engine, images):
    from zlibstream_amd import png_file_bound
    rows = images[2, 8][3]  # 65 x 129 RGB
    dims = (65, 129, 8, 2)
    want = _idat_reference(engine, [rows], [dims], [4], 6)[0]
    L = len(want)
    assert L > 8192 + 1, L
    sizes = [0, 1, 7, 13, 8192, L - 1, L, L + 1]
    for cb in sizes:
        rc, lens, st, bufs, offs, caps = _encode(engine, [rows], [dims], [4], 6, chunk_bytes=cb, offsets=[cb % 16])
        assert rc == ZS_OK and st == [ZS_OK], (cb, engine.last_error())
        assert lens[0] == png_file_bound(L, cb, 0)
        _check_file(bufs[0], offs[0], caps[0], lens[0], dims, rows, want, chunk_bytes=cb)


def test_encode_extra_chunks_pass_through_every_destination_residue(engine, images):
    rows_list, dims, extra = [], [], []
    types = (b"gAMA", b"tEXt", b"zTXt")
    for n in range(16):
        for count in (1, 2, 3):
            if count > 1 and n % 3:
                continue
            rows_list.append(images[6, 8][1])
            dims.append((3, 5, 8, 6))
            extra.append(b"".join(chunk(types[k], bytes(range(k, k + (n + k) % 16))) for k in range(count)))
    assert len({(33 + len(x) + 8) % 16 for x in extra}) == 16, "the IDAT data must land on every residue"
    want = _idat_reference(engine, rows_list, dims, [5] * len(dims), 6)
    rc, lens, st, bufs, offs, caps = _encode(engine, rows_list, dims, [5] * len(dims), 6, extra=extra, offsets=[0] * len(dims))
    assert rc == ZS_OK and st == [ZS_OK] * len(dims), engine.last_error()
    for i in range(len(dims)):
        _check_file(bufs[i], offs[i], caps[i], lens[i], dims[i], rows_list[i], want[i], extra=extra[i])


def test_encode_short_capacity_fails_for_that_image_only(engine, images):
    rows_list = [images[0, 8][2], images[6, 16][2], images[2, 8][4]]
    dims = [(33, 31, 8, 0), (33, 31, 16, 6), (1000, 3, 8, 2)]
    want = _idat_reference(engine, rows_list, dims, [5, 5, 5], 6)
    rc, lens, st, bufs, offs, caps = _encode(engine, rows_list, dims, [5, 5, 5], 6, chunk_bytes=100)
    assert rc == ZS_OK
    caps2 = [lens[0], lens[1] - 1, lens[2]]
    rc, lens2, st, bufs, offs, caps2 = _encode(engine, rows_list, dims, [5, 5, 5], 6, chunk_bytes=100, caps=caps2)
    assert rc == ZS_BUF_ERROR and st == [ZS_OK, ZS_BUF_ERROR, ZS_OK] and lens2 == lens
    assert bufs[1] == b"\xEE" * len(bufs[1]), "the image that does not fit was written to"
    for i in (0, 2):
        _check_file(bufs[i], offs[i], caps2[i], lens2[i], dims[i], rows_list[i], want[i], chunk_bytes=100)


def test_encode_bad_arguments_leave_status_untouched(engine, images):
    import ctypes
    from zlibstream_amd import _native
    L = _native.lib()
    rows = images[2, 8][1]
    d_px, d_out = _cuda(rows.tobytes()), _cuda(b"\xEE" * 4096)
    VP, I64, I32 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_int * 1
    good = dict(pixels=VP(d_px.data_ptr()), w=I64(3), h=I64(5), depth=I32(8), color=I32(2), filt=I32(0), extra=None, xlen=None, rpw=1, cb=0,
                out=VP(d_out.data_ptr()), cap=I64(4096), level=6, strategy=0)
    bad_extra = ctypes.create_string_buffer(b"\0\0\0\5tEXtab\0\0\0\0", 14)
    changes = [dict(w=I64(0)), dict(h=I64(0)), dict(w=I64(1 << 31)), dict(depth=I32(4)), dict(color=I32(5)), dict(depth=I32(16), color=I32(3)), dict(filt=I32(6)),
               dict(filt=I32(-1)), dict(rpw=-1), dict(cb=-1), dict(cb=1 << 31), dict(level=10), dict(strategy=9), dict(pixels=VP(None)), dict(out=VP(None)),
               dict(pixels=None), dict(w=None), dict(out=None), dict(cap=None), dict(extra=VP(ctypes.addressof(bad_extra)), xlen=I64(14)),
               dict(extra=VP(ctypes.addressof(bad_extra)), xlen=None), dict(extra=VP(None), xlen=I64(3)), dict(h=I64(1 << 30), w=I64(1 << 20))]
    for ch in changes:
        a = dict(good, **ch)
        st, out_len = I32(77), I64(99)
        rc = L.zs_png_encode_batch_device(engine.handle, 1, a["pixels"], a["w"], a["h"], a["depth"], a["color"], a["filt"], a["extra"], a["xlen"], a["rpw"], a["cb"],
                                          a["out"], a["cap"], out_len, st, a["level"], a["strategy"], 0, None)
        assert rc == ZS_STREAM_ERROR and st[0] == 77 and out_len[0] == 99, ch
    st = I32(77)
    assert L.zs_png_encode_batch_device(engine.handle, -1, good["pixels"], good["w"], good["h"], good["depth"], good["color"], good["filt"], None, None, 1, 0,
                                        good["out"], good["cap"], I64(0), st, 6, 0, 0, None) == ZS_STREAM_ERROR and st[0] == 77
    assert L.zs_png_encode_batch_device(engine.handle, 0, None, None, None, None, None, None, None, None, 1, 0, None, None, None, None, 6, 0, 0, None) == ZS_OK
    assert d_out.cpu().numpy().tobytes() == b"\xEE" * 4096


# ---------------------------------------------------------------- decode
@pytest.fixture(scope="module")
def hand_built():
    """files built here: every legal (color, depth) pair -- bits 1 to 64 -- interlaced and not, with every kind of IDAT split;
    -> (files, the raw scanlines each must give, what info must say)"""
    rng = np.random.default_rng(4410)
    files, want, infos = [], [], []
    gama, text = chunk(b"gAMA", b"\0\1\x86\xa0"), chunk(b"tEXt", b"Comment\0x")
    k = 0
    for color, depth in LEGAL:
        bits = depth * CHANNELS[color]
        for interlace in (0, 1):
            for w, h in ((1, 1), (3, 5), (33, 31), (65, 129)):
                rows = _random_rows(rng, w, h, bits) if k % 3 else _smooth_rows(w, h, bits)
                stream = zlib.compress(_payload(rng, rows, w, bits, interlace), 6 if k % 2 else 1)
                kind = k % 5
                if kind == 0:
                    cuts, label = (), "one chunk"
                elif kind == 1:
                    cuts, label = tuple(range(1, min(len(stream), 700))), "1-byte chunks"
                elif kind == 2:
                    cuts, label = (0, 0, 5, 5, 5, len(stream) // 2, len(stream), len(stream)), "zero-length chunks in between"
                elif kind == 3:
                    cuts, label = tuple(range(8192, len(stream), 8192)), "splits at 8192"
                else:
                    cuts, label = (len(stream) // 3,), "two chunks"
                anc = (k + k // 4) % 4  # (every shape meets every placement of the ancillary chunks)
                f = build_png(w, h, depth, color, interlace, stream, cuts, before=(gama,) if anc & 1 else (), after=(text,) if anc & 2 else ())
                n_idat = len([c for c in parse_png(f) if c[0] == b"IDAT"])
                files.append(f), want.append(rows.tobytes())
                infos.append(dict(width=w, height=h, bit_depth=depth, color_type=color, interlace=interlace, bits_per_pixel=bits, idat_bytes=len(stream),
                                  pixel_bytes=rows.size, n_idat=n_idat))
                k += 1
    # a stream long enough for splits at 8192 to be several chunks
    rows = _random_rows(rng, 300, 200, 24)
    stream = zlib.compress(_payload(rng, rows, 300, 24, 0), 6)
    assert len(stream) > 3 * 8192
    f = build_png(300, 200, 8, 2, 0, stream, tuple(range(8192, len(stream), 8192)), before=(gama, text), after=(text,))
    files.append(f), want.append(rows.tobytes())
    infos.append(dict(width=300, height=200, bit_depth=8, color_type=2, interlace=0, bits_per_pixel=24, idat_bytes=len(stream), pixel_bytes=rows.size,
                      n_idat=len(stream) // 8192 + 1))
    return files, want, infos


def test_decode_hand_built_files(engine, hand_built):
    files, want, infos = hand_built
    st, got_info, got = _decode_files(engine, files)
    assert st == [ZS_OK] * len(files), engine.last_error()
    assert got_info == infos
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[:len(w)].tobytes() == w, (i, infos[i])
        assert g[len(w):].tobytes() == b"\xEE" * GUARD, (i, "guard")


def _flip(f, i):
    return f[:i] + bytes([f[i] ^ 0x04]) + f[i + 1:]


def _pick(hand_built, **kw):
    files, want, infos = hand_built
    return [i for i, inf in enumerate(infos) if all(inf[k] == v for k, v in kw.items())]


@pytest.mark.parametrize("case", ["IDAT data", "IHDR", "truncated", "PLTE"])
def test_decode_one_broken_file_leaves_the_others_exact(engine, hand_built, case):
    files, want, infos = hand_built
    sel = _pick(hand_built, width=33, height=31)[:6] + [len(files) - 1]
    batch = [files[i] for i in sel]
    victim = 3
    f = batch[victim]
    chunks = parse_png(f)
    if case == "IDAT data":
        c = max((c for c in chunks if c[0] == b"IDAT"), key=lambda c: len(c[1]))
        batch[victim], needle = _flip(f, c[3] + 8 + len(c[1]) // 2), "CRC error in IDAT chunk at offset %d" % c[3]
    elif case == "IHDR":
        batch[victim], needle = _flip(f, 8 + 8 + 4 + 3), "CRC error in IHDR chunk at offset 8"  # height: 31 -> 27, still a legal IHDR
    elif case == "truncated":
        batch[victim], needle = f[:-5], "truncated chunk"
    else:
        i = _pick(hand_built, color_type=3, bit_depth=8, width=33)[0]
        f = files[i]
        plte = chunk(b"PLTE", bytes(range(30)))
        bad = chunk(b"PLTE", bytes(range(30)), crc=zlib.crc32(b"PLTE" + bytes(range(30))) ^ 1)
        sel[victim] = i
        batch[victim], needle = f[:33] + bad + f[33:], "CRC error in PLTE chunk at offset 33"
        batch.append(f[:33] + plte + f[33:]), sel.append(i)  # the same file with a good PLTE decodes
    st, _, got = _decode_files(engine, batch)
    assert st == [ZS_DATA_ERROR if j == victim else ZS_OK for j in range(len(batch))], engine.last_error()
    assert needle in engine.last_error() and "file %d" % victim in engine.last_error(), engine.last_error()
    for j, i in enumerate(sel):
        if j != victim:
            assert got[j][:len(want[i])].tobytes() == want[i], (case, j)
            assert got[j][len(want[i]):].tobytes() == b"\xEE" * GUARD


def test_decode_accepts_a_flipped_ancillary_crc_and_rejects_a_corrupt_stream(engine, hand_built):
    files, want, infos = hand_built
    i = next(i for i, f in enumerate(files) if b"gAMA" in f and infos[i]["width"] == 33)
    f = files[i]
    at = f.index(b"gAMA")
    anc = f[:at + 8] + struct.pack(">I", struct.unpack(">I", f[at + 8:at + 12])[0] ^ 0x10) + f[at + 12:]
    # a stream that is whole by its CRCs but does not inflate: the decode call's message comes through
    rows = np.frombuffer(want[i], dtype=np.uint8)
    inf = infos[i]
    broken = bytearray(zlib.compress(bytes(inf["height"] * (1 + inf["pixel_bytes"] // inf["height"])), 6))
    broken[-1] ^= 1  # the Adler-32 trailer
    bad = build_png(inf["width"], inf["height"], inf["bit_depth"], inf["color_type"], 0, bytes(broken))
    st, _, got = _decode_files(engine, [anc, bad, f])
    assert st == [ZS_OK, ZS_DATA_ERROR, ZS_OK], engine.last_error()
    assert "file 1" in engine.last_error() and "incorrect data check" in engine.last_error(), engine.last_error()
    assert got[0][:len(want[i])].tobytes() == want[i] and got[2][:len(want[i])].tobytes() == want[i]


def test_decode_short_capacity_and_bad_arguments(engine, hand_built):
    import ctypes
    from zlibstream_amd import _native
    files, want, infos = hand_built
    sel = _pick(hand_built, width=33, height=31, interlace=0)[:3]
    batch = [files[i] for i in sel]
    caps = [infos[sel[0]]["pixel_bytes"], infos[sel[1]]["pixel_bytes"] - 1, infos[sel[2]]["pixel_bytes"]]
    st, got_info, got = _decode_files(engine, batch, caps=caps)
    assert st == [ZS_OK, ZS_BUF_ERROR, ZS_OK] and got_info == [infos[i] for i in sel]
    assert got[1].tobytes() == b"\xEE" * len(got[1])
    for j in (0, 2):
        assert got[j][:caps[j]].tobytes() == want[sel[j]] and got[j][caps[j]:].tobytes() == b"\xEE" * GUARD
    L = _native.lib()
    f = batch[0]
    d_out = _cuda(b"\xEE" * 4096)
    VP, I64, I32 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_int * 1
    fp = VP(ctypes.cast(ctypes.c_char_p(f), ctypes.c_void_p).value)
    for a in ((-1, fp, I64(len(f)), VP(d_out.data_ptr()), I64(4096)), (1, None, I64(len(f)), VP(d_out.data_ptr()), I64(4096)),
              (1, fp, None, VP(d_out.data_ptr()), I64(4096)), (1, fp, I64(len(f)), None, I64(4096)), (1, fp, I64(len(f)), VP(d_out.data_ptr()), None),
              (1, VP(None), I64(len(f)), VP(d_out.data_ptr()), I64(4096)), (1, fp, I64(-1), VP(d_out.data_ptr()), I64(4096)),
              (1, fp, I64(len(f)), VP(None), I64(4096)), (1, fp, I64(len(f)), VP(d_out.data_ptr()), I64(-1))):
        st = I32(77)
        assert L.zs_png_decode_files_batch(engine.handle, a[0], a[1], a[2], a[3], a[4], None, st, None) == ZS_STREAM_ERROR and st[0] == 77
    assert L.zs_png_decode_files_batch(engine.handle, 0, None, None, None, None, None, None, None) == ZS_OK
    assert d_out.cpu().numpy().tobytes() == b"\xEE" * 4096


def test_round_trip_and_a_stream_of_the_caller(engine, images):
    import torch
    s = torch.cuda.Stream()
    rows_list, dims = [], []
    for (color, depth), imgs in images.items():
        for (w, h), r in zip(SHAPES, imgs):
            rows_list.append(r), dims.append((w, h, depth, color))
    filters = [i % 6 for i in range(len(dims))]
    rc, lens, st, bufs, offs, caps = _encode(engine, rows_list, dims, filters, 6, chunk_bytes=1000, stream=s.cuda_stream)
    assert rc == ZS_OK, engine.last_error()
    files = [b[o:o + n] for b, o, n in zip(bufs, offs, lens)]
    st, infos, got = _decode_files(engine, files, stream=s.cuda_stream)
    s.synchronize()
    assert st == [ZS_OK] * len(files), engine.last_error()
    for i, r in enumerate(rows_list):
        assert got[i][:r.size].tobytes() == r.tobytes(), dims[i]
        assert (infos[i]["width"], infos[i]["height"], infos[i]["bit_depth"], infos[i]["color_type"], infos[i]["interlace"]) == dims[i] + (0,)


def test_the_stage_timer_shows_the_framing(engine, images):
    engine.set_profiling(True)
    try:
        rc, lens, st, bufs, offs, caps = _encode(engine, [images[2, 8][3]], [(65, 129, 8, 2)], [5], 6)
        enc = engine.stage_ms()
        _decode_files(engine, [bufs[0][offs[0]:offs[0] + lens[0]]])
        dec = engine.stage_ms()
    finally:
        engine.set_profiling(False)
    assert rc == ZS_OK and enc.get("crc32_frame", 0) > 0 and dec.get("crc32_frame", 0) > 0, (enc, dec)


# ---------------------------------------------------------------- Pillow
PIL_CASES = (("L", 0, 8, 1), ("RGB", 2, 8, 3), ("RGBA", 6, 8, 4), ("I;16", 0, 16, 2), ("P", 3, 8, 1))


def test_pil_opens_what_the_encoder_writes(engine):
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    rng = np.random.default_rng(5150)
    w, h = 65, 129
    palette = bytes(rng.integers(0, 256, 768, dtype=np.uint8))
    rows_list = [rng.integers(0, 256, (h, w * nb), dtype=np.uint8) for _, _, _, nb in PIL_CASES]
    dims = [(w, h, depth, color) for _, color, depth, _ in PIL_CASES]
    extra = [chunk(b"PLTE", palette) if mode == "P" else b"" for mode, _, _, _ in PIL_CASES]
    rc, lens, st, bufs, offs, caps = _encode(engine, rows_list, dims, [5] * len(dims), 6, chunk_bytes=8192, extra=extra)
    assert rc == ZS_OK, engine.last_error()
    for (mode, color, depth, nb), rows, b, o, n in zip(PIL_CASES, rows_list, bufs, offs, lens):
        im = Image.open(io.BytesIO(b[o:o + n]))
        im.load()
        assert im.size == (w, h)
        if mode == "I;16":
            got = np.asarray(im).astype(">u2").tobytes()  # PNG samples are big-endian
            assert im.mode.startswith("I")
        else:
            assert im.mode == mode
            got = np.asarray(im).tobytes()
        assert got == rows.tobytes(), mode
        if mode == "P":
            assert bytes(im.getpalette()) == palette


@pytest.mark.parametrize("optimize", [False, True])
def test_decoder_reads_what_pil_saves(engine, optimize):
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    rng = np.random.default_rng(5151)
    w, h = 300, 200
    y, x = np.mgrid[0:h, 0:w]
    files, want = [], []
    for mode, color, depth, nb in PIL_CASES:
        if mode == "I;16":
            a = ((x * 257 + y * 31) & 0xFFFF).astype(np.uint16)
            im, raw = Image.frombytes("I;16", (w, h), a.astype("<u2").tobytes()), a.astype(">u2").tobytes()  # (PNG samples are big-endian)
        elif mode == "P":
            a = ((x // 3 + y // 2) & 255).astype(np.uint8)
            im = Image.frombytes("P", (w, h), a.tobytes())
            im.putpalette(bytes(rng.integers(0, 256, 768, dtype=np.uint8)))
            raw = a.tobytes()
        else:
            a = np.stack([((x * (c + 1) + y * 2 + rng.integers(0, 3, x.shape)) & 255) for c in range(nb)], axis=2).astype(np.uint8)
            im, raw = Image.frombytes(mode, (w, h), a.tobytes()), a.tobytes()
        buf = io.BytesIO()
        im.save(buf, format="PNG", optimize=optimize)
        files.append(buf.getvalue()), want.append((raw, color, depth))
    st, infos, got = _decode_files(engine, files)
    assert st == [ZS_OK] * len(files), engine.last_error()
    for (raw, color, depth), inf, g in zip(want, infos, got):
        assert (inf["color_type"], inf["bit_depth"], inf["width"], inf["height"]) == (color, depth, w, h)
        assert g[:len(raw)].tobytes() == raw, (color, depth)
