"""Interlaced PNG encoding on the device: the Adam7 split (zs_png_adam7_split_batch_device), pixels to IDAT payloads
(zs_png_idat_interlace_batch_device) and pixels to files (zs_png_encode_interlace_batch_device).  The references are a numpy
restatement of PNG specification 8.2 by slices and of 9.2, Python's struct, zlib.crc32 and zlib.decompress, the oracle's Write
loop, and the library's own decode side; every comparison is exact."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZS_OK, ZS_STREAM_ERROR, ZS_BUF_ERROR = 0, -2, -5
SIG = b"\x89PNG\r\n\x1a\n"
SHAPES = ((1, 1), (3, 5), (33, 31), (65, 129), (1000, 3), (4, 4), (5, 1), (1, 9), (8, 8))
BITS = (1, 2, 4, 8, 16, 24, 32, 48, 64)
# PNG specification table 11.1
LEGAL = [(c, d) for c, ds in ((0, (1, 2, 4, 8, 16)), (2, (8, 16)), (3, (1, 2, 4, 8)), (4, (8, 16)), (6, (8, 16))) for d in ds]
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
ONE_PAIR_PER_BITS = ((0, 1), (0, 2), (3, 4), (0, 8), (4, 8), (2, 8), (6, 8), (2, 16), (6, 16))  # 1, 2, 4, 8, 16, 24, 32, 48, 64 bits
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))  # xstart, ystart, xstep, ystep
GUARD = 64


# ---------------------------------------------------------------- the specification, restated
def _row_bytes(w, bits):
    return (w * bits + 7) // 8


def _rows(rng, w, h, bits, smooth=False):
    """(h, row_bytes) raw scanlines whose padding bits are all ones, and the same with the padding bits cleared"""
    if smooth:
        y, x = np.mgrid[0:h, 0:_row_bytes(w, bits)]
        rows = ((x // max(1, bits // 8)) * 3 + y * 5 + (x % max(1, bits // 8)) * 40).astype(np.uint8)
    else:
        rows = rng.integers(0, 256, (h, _row_bytes(w, bits)), dtype=np.uint8)
    clear = rows.copy()
    used = (w * bits) % 8
    if used:
        rows[:, -1] |= 0xFF >> used
        clear[:, -1] &= (0xFF00 >> used) & 0xFF
    return rows, clear


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


def _passes(rows, w, bits):
    """PNG specification 8.2 by slices: the present passes' scanlines, padding bits zero"""
    px = _unpack(rows, w, bits)
    out = []
    for xs, ys, xst, yst in ADAM7:
        sub = px[ys::yst, xs::xst]
        if sub.shape[0] and sub.shape[1]:
            out.append(_pack(sub, bits))
    return out


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


def _np_payload(rows, w, bits, ftype):
    """the interlaced IDAT payload with one fixed filter type: filtering restarts at every pass"""
    return b"".join(_filter_rows(p, max(1, bits // 8), [ftype] * p.shape[0]).tobytes() for p in _passes(rows, w, bits))


def _write_ends(row_sizes, rows_per_write):
    """the cumulative Write ends of a stream whose rows have the given sizes; None: one Write"""
    if rows_per_write == 0 or rows_per_write >= len(row_sizes):
        return None
    cum = np.cumsum(row_sizes)
    return [int(cum[r - 1]) for r in range(rows_per_write, len(row_sizes), rows_per_write)] + [int(cum[-1])]


def _stream_row_sizes(w, h, bits, interlace):
    from zlibstream_amd import png_idat_layout
    _, rb, rows = png_idat_layout(w, h, bits, interlace)
    return [b + 1 for b, r in zip(rb, rows) for _ in range(r)]


def chunk(ctype, data):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data))


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


class Placed:
    """byte strings at odd offsets inside 0xEE-filled device tensors of their own, GUARD bytes on both sides"""

    def __init__(self, items, sizes=None):
        import torch
        self.sizes = [len(x) for x in items] if sizes is None else list(sizes)
        self.off = [GUARD + 1 + 2 * (i % 8) for i in range(len(self.sizes))]
        self.t = []
        for i, (o, n) in enumerate(zip(self.off, self.sizes)):
            host = np.full(o + n + GUARD, 0xEE, dtype=np.uint8)
            if sizes is None:
                host[o:o + n] = np.frombuffer(bytes(items[i]), dtype=np.uint8)
            self.t.append(torch.from_numpy(host).cuda())
        torch.cuda.synchronize()  # torch fills on its own stream; the engine's stream does not wait for that one

    @property
    def ptrs(self):
        return [t.data_ptr() + o for t, o in zip(self.t, self.off)]

    def get(self, i, n=None):
        """the first n bytes of item i, after checking that nothing outside them (n: outside the item's size) was written"""
        host = self.t[i].cpu().numpy().tobytes()
        o, size = self.off[i], self.sizes[i] if n is None else n
        assert host[:o] == b"\xEE" * o and host[o + size:] == b"\xEE" * (len(host) - o - size), "bytes outside the output were written"
        return host[o:o + size]


def _idat(engine, rows_list, dims, interlace, filters, level, rows_per_write=1, caps=None):
    """png_idat_interlace_batch_device -> (rc, statuses, the streams, the output buffers); dims: (w, h, bits)"""
    from zlibstream_amd import deflate_bound, png_idat_interlace_batch_device, png_idat_layout
    src = Placed([r.tobytes() for r in rows_list])
    if caps is None:
        caps = [deflate_bound(png_idat_layout(w, h, b, il)[0]) for (w, h, b), il in zip(dims, interlace or [0] * len(dims))]
    out = Placed(None, sizes=caps)
    rc, lens, st = png_idat_interlace_batch_device(engine, src.ptrs, [d[0] for d in dims], [d[1] for d in dims], [d[2] for d in dims], interlace, filters,
                                                   out.ptrs, caps, rows_per_write=rows_per_write, level=level, return_status=True)
    # (the deflate call may write anywhere inside a stream's capacity; nothing outside it)
    return rc, st, [out.get(i)[:n] if s == ZS_OK else None for i, (n, s) in enumerate(zip(lens, st))], lens, out


def _encode(engine, rows_list, dims, interlace, filters, level, chunk_bytes=0, extra=None, caps=None, rows_per_write=1):
    """png_encode_interlace_batch_device -> (rc, statuses, the files, lengths, the output buffers); dims: (w, h, depth, color)"""
    from zlibstream_amd import deflate_bound, png_encode_interlace_batch_device, png_file_bound, png_idat_layout
    src = Placed([r.tobytes() for r in rows_list])
    if caps is None:
        ils = interlace or [0] * len(dims)
        caps = [png_file_bound(deflate_bound(png_idat_layout(w, h, d * CHANNELS[c], il)[0]), chunk_bytes, len(extra[i]) if extra else 0)
                for i, ((w, h, d, c), il) in enumerate(zip(dims, ils))]
    out = Placed(None, sizes=caps)
    rc, lens, st = png_encode_interlace_batch_device(engine, src.ptrs, [d[0] for d in dims], [d[1] for d in dims], [d[2] for d in dims],
                                                     [d[3] for d in dims], filters, out.ptrs, caps, interlace=interlace, extra=extra,
                                                     rows_per_write=rows_per_write, idat_chunk_bytes=chunk_bytes, level=level, return_status=True)
    return rc, st, [out.get(i, n) if s == ZS_OK else None for i, (n, s) in enumerate(zip(lens, st))], lens, out


@pytest.fixture(scope="module")
def images():
    """bits -> [(rows with their padding bits set, rows with them cleared)] for SHAPES, made once and left unchanged"""
    rng = np.random.default_rng(8802)
    return {bits: [_rows(rng, w, h, bits, smooth=(w + h) % 2 == 1) for w, h in SHAPES] for bits in BITS}


# ---------------------------------------------------------------- the split
@pytest.mark.parametrize("bits", BITS)
def test_split_equals_the_slices_and_merge_inverts_it(engine, images, bits):
    from zlibstream_amd import png_adam7_merge_batch_device, png_adam7_split_batch_device
    dirty = [images[bits][k][0] for k in range(len(SHAPES))]
    clean = [images[bits][k][1] for k in range(len(SHAPES))]
    want = [b"".join(p.tobytes() for p in _passes(r, w, bits)) for r, (w, h) in zip(dirty, SHAPES)]
    ws, hs = [s[0] for s in SHAPES], [s[1] for s in SHAPES]

    def check(sel):
        src = Placed([dirty[k].tobytes() for k in sel])
        out = Placed(None, sizes=[len(want[k]) for k in sel])
        png_adam7_split_batch_device(engine, src.ptrs, [ws[k] for k in sel], [hs[k] for k in sel], [bits] * len(sel), out.ptrs)
        for i, k in enumerate(sel):
            assert out.get(i) == want[k], (bits, SHAPES[k], "split")
            assert src.get(i) == dirty[k].tobytes(), (bits, SHAPES[k], "the input changed")
        back = Placed(None, sizes=[clean[k].size for k in sel])
        png_adam7_merge_batch_device(engine, out.ptrs, [ws[k] for k in sel], [hs[k] for k in sel], [bits] * len(sel), back.ptrs)
        for i, k in enumerate(sel):
            assert back.get(i) == clean[k].tobytes(), (bits, SHAPES[k], "merge of the split")

    for k in range(len(SHAPES)):  # one image per call
        check([k])
    check(list(range(len(SHAPES))))  # all in one call: the flat row list crosses image and pass boundaries


# ---------------------------------------------------------------- IDAT payloads
def _composition_reference(engine, rows_list, dims, filters, level, rows_per_write):
    """what zs_deflate_writes_batch_device returns for the payload that zs_png_filter_batch_device makes of the numpy-made passes,
    laid back to back, with the Write ends of the interlaced stream -> (streams, payloads)"""
    from zlibstream_amd import deflate_bound, png_filter_batch_device
    import torch
    f_in, f_rb, f_h, f_bpp, f_filter, f_at, sizes = [], [], [], [], [], [], []
    for rows, (w, h, bits), f in zip(rows_list, dims, filters):
        at = 0
        for p in _passes(rows, w, bits):
            f_in.append(p.tobytes()), f_rb.append(p.shape[1]), f_h.append(p.shape[0]), f_bpp.append(max(1, bits // 8)), f_filter.append(f)
            f_at.append((len(sizes), at))
            at += p.shape[0] * (p.shape[1] + 1)
        sizes.append(at)
    src = Placed(f_in)
    pay = Placed(None, sizes=sizes)
    png_filter_batch_device(engine, src.ptrs, f_rb, f_h, f_bpp, f_filter, [pay.ptrs[i] + at for i, at in f_at])
    payloads = [pay.get(i) for i in range(len(sizes))]
    ends = [_write_ends(_stream_row_sizes(w, h, bits, 1), rows_per_write) for w, h, bits in dims]
    caps = [deflate_bound(n) for n in sizes]
    z = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    torch.cuda.synchronize()
    lens = engine.deflate_writes_batch_device(pay.ptrs, sizes, ends, [t.data_ptr() for t in z], caps, level=level)
    return [t[:n].cpu().numpy().tobytes() for t, n in zip(z, lens)], payloads


@pytest.mark.parametrize("color,depth", LEGAL)
def test_idat_every_legal_pair_and_filter_interlaced_and_not_in_one_call(engine, images, color, depth):
    from zlibstream_amd import deflate_bound, png_idat_batch_device
    import torch
    bits = depth * CHANNELS[color]
    rows_list, dims, il, filters = [], [], [], []
    for k, (w, h) in enumerate(SHAPES):
        for f in range(6):
            rows_list.append(images[bits][k][0]), dims.append((w, h, bits)), il.append(1), filters.append(f)
        rows_list.append(images[bits][k][0]), dims.append((w, h, bits)), il.append(0), filters.append(k % 6)  # a non-interlaced one in between
    rc, st, streams, _, _ = _idat(engine, rows_list, dims, il, filters, 6)
    assert rc == ZS_OK and st == [ZS_OK] * len(dims), engine.last_error()
    inter = [i for i in range(len(dims)) if il[i]]
    want, payloads = _composition_reference(engine, [rows_list[i] for i in inter], [dims[i] for i in inter], [filters[i] for i in inter], 6, 1)
    for j, i in enumerate(inter):
        assert streams[i] == want[j], (dims[i], filters[i], "not the deflate call's stream for the filtered passes")
        if filters[i] < 5:
            w, h, _ = dims[i]
            assert zlib.decompress(streams[i]) == _np_payload(rows_list[i], w, bits, filters[i]), (dims[i], filters[i])
        else:
            assert zlib.decompress(streams[i]) == payloads[j]
    # the non-interlaced images of the same call: png_idat_batch_device's streams
    plain = [i for i in range(len(dims)) if not il[i]]
    src = Placed([rows_list[i].tobytes() for i in plain])
    caps = [deflate_bound(dims[i][1] * (_row_bytes(dims[i][0], bits) + 1)) for i in plain]
    z = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    torch.cuda.synchronize()
    lens = png_idat_batch_device(engine, src.ptrs, [_row_bytes(dims[i][0], bits) for i in plain], [dims[i][1] for i in plain], [max(1, bits // 8)] * len(plain),
                                 [filters[i] for i in plain], [t.data_ptr() for t in z], caps, rows_per_write=1, level=6)
    for j, i in enumerate(plain):
        assert streams[i] == z[j][:lens[j]].cpu().numpy().tobytes(), (dims[i], "not png_idat_batch_device's stream")


@pytest.mark.parametrize("level", [1, 6])
@pytest.mark.parametrize("rows_per_write", [0, 1, 3])
def test_idat_streams_equal_the_oracle_write_loop(engine, oracle, images, rows_per_write, level):
    """one pair at each bits value; 3 rows a Write makes Writes straddle pass boundaries"""
    rows_list, dims, filters = [], [], []
    for color, depth in ONE_PAIR_PER_BITS:
        bits = depth * CHANNELS[color]
        for k, (w, h) in enumerate(SHAPES):
            rows_list.append(images[bits][k][0]), dims.append((w, h, bits)), filters.append((k + bits) % 5)
    rc, st, streams, _, _ = _idat(engine, rows_list, dims, [1] * len(dims), filters, level, rows_per_write=rows_per_write)
    assert rc == ZS_OK and st == [ZS_OK] * len(dims), engine.last_error()
    straddles = 0
    for rows, (w, h, bits), f, z in zip(rows_list, dims, filters, streams):
        payload = _np_payload(rows, w, bits, f)
        sizes = _stream_row_sizes(w, h, bits, 1)
        ends = _write_ends(sizes, rows_per_write)
        chunks = [e - s for s, e in zip([0] + ends[:-1], ends)] if ends else None
        assert z == oracle.compress(payload, level, chunks=chunks), (w, h, bits, f)
        if ends and rows_per_write == 3:
            from zlibstream_amd import png_idat_layout
            _, rb, nrows = png_idat_layout(w, h, bits, 1)
            bounds = set(np.cumsum([r * (b + 1) for b, r in zip(rb, nrows) if r]).tolist())
            straddles += any(e not in bounds and any(s < x < e for x in bounds) for s, e in zip([0] + ends[:-1], ends))
    assert rows_per_write != 3 or straddles > 0


# ---------------------------------------------------------------- files
def _check_file(f, dims, interlace, want_stream, extra=b"", chunk_bytes=0):
    w, h, depth, color = dims
    chunks = parse_png(f)
    for t, data, crc, at in chunks:
        assert crc == zlib.crc32(t + data), (t, at)
    assert chunks[0][0] == b"IHDR" and chunks[0][1] == struct.pack(">IIBBBBB", w, h, depth, color, 0, 0, interlace)
    assert chunks[-1][0] == b"IEND" and chunks[-1][1] == b""
    first = next(i for i, c in enumerate(chunks) if c[0] == b"IDAT")
    assert f[33:chunks[first][3]] == extra, "the caller's chunks are not verbatim between IHDR and IDAT"
    idat = chunks[first:-1]
    assert all(c[0] == b"IDAT" for c in idat)
    stream = b"".join(c[1] for c in idat)
    assert stream == want_stream, "the IDAT data is not the IDAT call's stream"
    if chunk_bytes:
        assert [len(c[1]) for c in idat] == [min(chunk_bytes, len(stream) - a) for a in range(0, len(stream), chunk_bytes)]
    else:
        assert len(idat) == 1


PLTE = chunk(b"PLTE", bytes((7 * i + 3) & 255 for i in range(768)))
GAMA = chunk(b"gAMA", b"\0\1\x86\xa0")


def _file_batch(images):
    rows_list, clean, dims, filters, extra = [], [], [], [], []
    for color, depth in LEGAL:
        bits = depth * CHANNELS[color]
        for k, (w, h) in enumerate(SHAPES):
            rows_list.append(images[bits][k][0]), clean.append(images[bits][k][1]), dims.append((w, h, depth, color))
            filters.append(len(dims) % 6)
            extra.append((PLTE if color == 3 else b"") + (GAMA if k % 2 else b""))
    return rows_list, clean, dims, filters, extra


@pytest.mark.parametrize("chunk_bytes", [0, 37])
def test_files_every_legal_pair_interlaced(engine, images, chunk_bytes):
    from zlibstream_amd import png_decode_files_batch
    rows_list, clean, dims, filters, extra = _file_batch(images)
    n = len(dims)
    rc, st, files, lens, _ = _encode(engine, rows_list, dims, [1] * n, filters, 6, chunk_bytes=chunk_bytes, extra=extra)
    assert rc == ZS_OK and st == [ZS_OK] * n, engine.last_error()
    rc, st, want, _, _ = _idat(engine, rows_list, [(w, h, d * CHANNELS[c]) for w, h, d, c in dims], [1] * n, filters, 6)
    assert rc == ZS_OK
    assert any(len(z) > 37 for z in want)  # (the small chunk size cuts mid-stream)
    for i in range(n):
        _check_file(files[i], dims[i], 1, want[i], extra=extra[i], chunk_bytes=chunk_bytes)
    # the library's own decoder gives the pixels back, padding bits cleared
    out = Placed(None, sizes=[r.size for r in clean])
    st, infos = png_decode_files_batch(engine, files, out.ptrs, out.sizes)
    assert st == [ZS_OK] * n, engine.last_error()
    for i in range(n):
        assert out.get(i) == clean[i].tobytes(), dims[i]
        assert (infos[i]["width"], infos[i]["height"], infos[i]["bit_depth"], infos[i]["color_type"], infos[i]["interlace"]) == dims[i] + (1,)


def test_files_decode_to_rgba_like_the_originals_expanded(engine, images):
    """a palette pair with tRNS: files -> RGBA agrees with the expansion of the original scanlines"""
    import torch
    from zlibstream_amd import png_decode_files_rgba_batch, png_expand_batch_device
    color, depth = 3, 4
    plte, trns = bytes((11 * i + 5) & 255 for i in range(48)), bytes((37 * i) & 255 for i in range(9))
    extra = chunk(b"PLTE", plte) + chunk(b"tRNS", trns)
    n = len(SHAPES)
    rows_list, clean = [images[4][k][0] for k in range(n)], [images[4][k][1] for k in range(n)]
    dims = [(w, h, depth, color) for w, h in SHAPES]
    rc, st, files, _, _ = _encode(engine, rows_list, dims, [1] * n, [5] * n, 6, extra=[extra] * n)
    assert rc == ZS_OK and st == [ZS_OK] * n, engine.last_error()
    got = [torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for w, h in SHAPES]
    want = [torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for w, h in SHAPES]
    src = [_cuda(r.tobytes()) for r in clean]
    torch.cuda.synchronize()
    st, _ = png_decode_files_rgba_batch(engine, files, [t.data_ptr() for t in got], [t.numel() for t in got])
    assert st == [ZS_OK] * n, engine.last_error()
    png_expand_batch_device(engine, [t.data_ptr() for t in src], [s[0] for s in SHAPES], [s[1] for s in SHAPES], [depth] * n, [color] * n,
                            [t.data_ptr() for t in want], plte=[plte] * n, trns=[trns] * n)
    for g, w_, s in zip(got, want, SHAPES):
        assert g.cpu().numpy().tobytes() == w_.cpu().numpy().tobytes(), s


def test_files_without_interlace_are_the_plain_encoder_s(engine, images):
    from zlibstream_amd import png_encode_batch_device
    rows_list, clean, dims, filters, extra = _file_batch(images)
    sel = list(range(0, len(dims), 7))
    rows_list, dims, filters, extra = [rows_list[i] for i in sel], [dims[i] for i in sel], [filters[i] for i in sel], [extra[i] for i in sel]
    src = Placed([r.tobytes() for r in rows_list])
    rc, st, none_files, lens, out = _encode(engine, rows_list, dims, None, filters, 6, chunk_bytes=100, extra=extra)
    assert rc == ZS_OK and st == [ZS_OK] * len(dims), engine.last_error()
    rc, st, zero_files, _, _ = _encode(engine, rows_list, dims, [0] * len(dims), filters, 6, chunk_bytes=100, extra=extra)
    assert rc == ZS_OK and st == [ZS_OK] * len(dims), engine.last_error()
    plain = Placed(None, sizes=out.sizes)
    rc, plens, st = png_encode_batch_device(engine, src.ptrs, [d[0] for d in dims], [d[1] for d in dims], [d[2] for d in dims], [d[3] for d in dims], filters,
                                            plain.ptrs, plain.sizes, extra=extra, rows_per_write=1, idat_chunk_bytes=100, level=6, return_status=True)
    assert rc == ZS_OK and plens == lens
    for i in range(len(dims)):
        assert none_files[i] == zero_files[i] == plain.get(i, plens[i]), dims[i]


def test_pil_opens_the_interlaced_files(engine):
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    rng = np.random.default_rng(5152)
    w, h = 65, 129
    cases = (("L", 0, 8, 1), ("RGB", 2, 8, 3), ("RGBA", 6, 8, 4), ("P", 3, 8, 1))
    palette = bytes(rng.integers(0, 256, 768, dtype=np.uint8))
    rows_list = [rng.integers(0, 256, (h, w * nb), dtype=np.uint8) for _, _, _, nb in cases]
    dims = [(w, h, depth, color) for _, color, depth, _ in cases]
    extra = [chunk(b"PLTE", palette) if mode == "P" else b"" for mode, _, _, _ in cases]
    rc, st, files, _, _ = _encode(engine, rows_list, dims, [1] * len(dims), [5] * len(dims), 6, chunk_bytes=8192, extra=extra)
    assert rc == ZS_OK, engine.last_error()
    for (mode, _, _, _), rows, f in zip(cases, rows_list, files):
        im = Image.open(io.BytesIO(f))
        im.load()
        assert im.size == (w, h) and im.mode == mode
        assert np.asarray(im).tobytes() == rows.tobytes(), mode


# ---------------------------------------------------------------- errors
def test_a_capacity_one_byte_short_fails_for_that_image_only(engine, images):
    rows_list = [images[8][2][0], images[32][2][0], images[1][3][0]]
    idims, fdims = [(33, 31, 8), (33, 31, 32), (65, 129, 1)], [(33, 31, 8, 0), (33, 31, 8, 6), (65, 129, 1, 0)]
    il = [1, 1, 1]
    rc, st, want, lens, _ = _idat(engine, rows_list, idims, il, [5] * 3, 6)
    assert rc == ZS_OK
    from zlibstream_amd import deflate_bound
    rc, st, got, lens2, out = _idat(engine, rows_list, idims, il, [5] * 3, 6, caps=[deflate_bound(lens[0]), lens[1] - 1, deflate_bound(lens[2])])
    assert rc == ZS_BUF_ERROR and st == [ZS_OK, ZS_BUF_ERROR, ZS_OK]
    assert got[0] == want[0] and got[2] == want[2]
    out.get(1, lens[1] - 1)  # (whatever the short stream's buffer holds, nothing outside it was written)
    rc, st, files, flens, _ = _encode(engine, rows_list, fdims, il, [5] * 3, 6, chunk_bytes=100)
    assert rc == ZS_OK
    rc, st, files2, flens2, out = _encode(engine, rows_list, fdims, il, [5] * 3, 6, chunk_bytes=100, caps=[flens[0], flens[1] - 1, flens[2]])
    assert rc == ZS_BUF_ERROR and st == [ZS_OK, ZS_BUF_ERROR, ZS_OK] and flens2 == flens
    assert files2[0] == files[0] and files2[2] == files[2]
    assert out.get(1, 0) == b"", "the image that does not fit was written to"


def test_bad_arguments_leave_status_and_lengths_untouched(engine, images):
    from zlibstream_amd import _native
    L = _native.lib()
    rows = images[24][1][0]  # 3 x 5 RGB
    d_px, d_out = _cuda(rows.tobytes()), _cuda(b"\xEE" * 4096)
    VP, I64, I32 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_int * 1
    good = dict(pixels=VP(d_px.data_ptr()), w=I64(3), h=I64(5), depth=I32(8), color=I32(2), bits=I32(24), il=I32(1), filt=I32(0), rpw=1, out=VP(d_out.data_ptr()),
                cap=I64(4096))
    enc_changes = [dict(il=I32(2)), dict(il=I32(-1)), dict(pixels=None), dict(w=None), dict(h=None), dict(depth=None), dict(color=None), dict(filt=None),
                   dict(out=None), dict(cap=None), dict(depth=I32(4)), dict(depth=I32(16), color=I32(3)), dict(color=I32(5)), dict(rpw=-1), dict(pixels=VP(None)),
                   dict(out=VP(None)), dict(w=I64(0)), dict(filt=I32(6))]
    for ch in enc_changes:
        a = dict(good, **ch)
        st, out_len = I32(77), I64(99)
        rc = L.zs_png_encode_interlace_batch_device(engine.handle, 1, a["pixels"], a["w"], a["h"], a["depth"], a["color"], a["filt"], a["il"], None, None, a["rpw"], 0,
                                                    a["out"], a["cap"], out_len, st, 6, 0, 0, None)
        assert rc == ZS_STREAM_ERROR and st[0] == 77 and out_len[0] == 99, ch
    idat_changes = [dict(il=I32(2)), dict(il=I32(-1)), dict(pixels=None), dict(w=None), dict(h=None), dict(bits=None), dict(filt=None), dict(out=None),
                    dict(cap=None), dict(bits=I32(12)), dict(bits=I32(40)), dict(rpw=-1), dict(pixels=VP(None)), dict(w=I64(0)), dict(h=I64(1 << 31)),
                    dict(filt=I32(6)), dict(w=I64(1 << 15), h=I64(1 << 14), bits=I32(32)), dict(out=VP(None)), dict(cap=I64(-1))]
    for ch in idat_changes:
        a = dict(good, **ch)
        st, out_len = I32(77), I64(99)
        rc = L.zs_png_idat_interlace_batch_device(engine.handle, 1, a["pixels"], a["w"], a["h"], a["bits"], a["il"], a["filt"], a["rpw"], a["out"], a["cap"], out_len,
                                                  st, 6, 0, 0, None)
        assert rc == ZS_STREAM_ERROR and st[0] == 77 and out_len[0] == 99, ch
    for ch in (dict(pixels=None), dict(w=None), dict(bits=None), dict(out=None), dict(bits=I32(12)), dict(w=I64(0)), dict(pixels=VP(None)), dict(out=VP(None))):
        a = dict(good, **ch)
        assert L.zs_png_adam7_split_batch_device(engine.handle, 1, a["pixels"], a["w"], a["h"], a["bits"], a["out"], None) == ZS_STREAM_ERROR, ch
    st = I32(77)
    assert L.zs_png_encode_interlace_batch_device(engine.handle, -1, good["pixels"], good["w"], good["h"], good["depth"], good["color"], good["filt"], good["il"],
                                                  None, None, 1, 0, good["out"], good["cap"], I64(0), st, 6, 0, 0, None) == ZS_STREAM_ERROR and st[0] == 77
    assert L.zs_png_encode_interlace_batch_device(engine.handle, 0, None, None, None, None, None, None, None, None, None, 1, 0, None, None, None, None, 6, 0, 0,
                                                  None) == ZS_OK
    assert L.zs_png_idat_interlace_batch_device(engine.handle, 0, None, None, None, None, None, None, 1, None, None, None, None, 6, 0, 0, None) == ZS_OK
    assert L.zs_png_adam7_split_batch_device(engine.handle, 0, None, None, None, None, None, None) == ZS_OK
    assert d_out.cpu().numpy().tobytes() == b"\xEE" * 4096
    # a null interlace array is "all 0": the plain encoder's file
    st, out_len = I32(77), I64(99)
    rc = L.zs_png_encode_interlace_batch_device(engine.handle, 1, good["pixels"], good["w"], good["h"], good["depth"], good["color"], good["filt"], None, None, None,
                                                1, 0, good["out"], good["cap"], out_len, st, 6, 0, 0, None)
    assert rc == ZS_OK and st[0] == ZS_OK
    f = d_out.cpu().numpy().tobytes()[:out_len[0]]
    assert parse_png(f)[0][1] == struct.pack(">IIBBBBB", 3, 5, 8, 2, 0, 0, 0)


def test_the_stage_timer_shows_the_split(engine, images):
    from zlibstream_amd import png_adam7_split_batch_device
    engine.set_profiling(True)
    try:
        rc, st, _, _, _ = _encode(engine, [images[24][3][0]], [(65, 129, 8, 2)], [1], [5], 6)
        enc = engine.stage_ms()
        src, out = Placed([images[24][3][0].tobytes()]), Placed(None, sizes=[images[24][3][0].size])
        png_adam7_split_batch_device(engine, src.ptrs, [65], [129], [24], out.ptrs)
        alone = engine.stage_ms()
    finally:
        engine.set_profiling(False)
    assert rc == ZS_OK and enc.get("png_split", 0) > 0 and enc.get("crc32_frame", 0) > 0 and alone.get("png_split", 0) > 0, (enc, alone)
