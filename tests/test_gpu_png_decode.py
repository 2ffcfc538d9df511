"""IDAT payloads to pixels on the device (zs_png_decode_batch_device: inflate, KU, and for interlaced images the Adam7
interleave KA) and the interleave alone (zs_png_adam7_merge_batch_device).  Inputs are made here: pixels forward-filtered with
numpy, split into passes by a restatement of the table of PNG specification 8.2 (slices xstart::xstep), compressed with
Python's zlib.  The shapes are the smallest at which KA and the pass bookkeeping can go wrong: absent passes, rows shorter
than a byte, rows that end mid-byte, the 64-pixel wave edge, and one row longer than what a wave's 64 lanes store in one
step at any depth (1 KiB, 256 bytes below 8 bits: 2100 pixels cross it everywhere).  Every comparison is exact."""
import ctypes
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZS_OK, ZS_STREAM_ERROR, ZS_DATA_ERROR = 0, -2, -3
BITS = (1, 2, 4, 8, 16, 24, 32, 48, 64)
SHAPES = ((1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (4, 4), (5, 3), (7, 7), (8, 8), (9, 9), (13, 17), (33, 31), (64, 64), (65, 129), (257, 63),
          (1000, 3), (2100, 2))
# PNG specification 8.2
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))  # xstart, ystart, xstep, ystep


# ---------------------------------------------------------------- the specification, restated with numpy
def _pack(px, bits):
    """px: (h, w) pixel values below 8 bits, (h, w, bits / 8) bytes otherwise -> (h, row_bytes) raw scanlines, leftmost pixel in
    the high bits, padding bits zero"""
    if bits >= 8:
        return np.ascontiguousarray(px).reshape(px.shape[0], -1)
    b = (px[:, :, None] >> np.arange(bits - 1, -1, -1)) & 1
    return np.packbits(b.reshape(px.shape[0], -1).astype(np.uint8), axis=1)


def _unpack(rows, w, bits):
    if bits >= 8:
        return rows.reshape(rows.shape[0], w, bits // 8)
    b = np.unpackbits(rows, axis=1)[:, :w * bits].reshape(rows.shape[0], w, bits)
    return (b * (1 << np.arange(bits - 1, -1, -1))).sum(axis=2).astype(np.uint8)


def _random_px(rng, w, h, bits):
    if bits >= 8:
        return rng.integers(0, 256, (h, w, bits // 8), dtype=np.uint8)
    return rng.integers(0, 1 << bits, (h, w), dtype=np.uint8)


def _smooth_px(w, h, channels):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([((x * (c + 1) + y * (3 - c)) // 4 + 16 * c) & 255 for c in range(channels)], axis=2).astype(np.uint8)


def _passes(px):
    """the present passes of an image, as pixel arrays, in pass order (with their numbers 1..7)"""
    out = []
    for p, (xs, ys, xst, yst) in enumerate(ADAM7):
        sub = px[ys::yst, xs::xst]
        if sub.shape[0] and sub.shape[1]:
            out.append((p + 1, sub))
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


def _payload(rng, px, bits, interlace):
    """the IDAT payload before compression: random filter types per row (per pass row)"""
    bpp = max(1, bits // 8)
    parts = _passes(px) if interlace else [(0, px)]
    return b"".join(_filter_rows(_pack(sub, bits), bpp, rng.integers(0, 5, sub.shape[0])).tobytes() for _, sub in parts)


# ---------------------------------------------------------------- device plumbing
def _cuda(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def _decode(engine, streams, shapes, bits, interlace, stream=None):
    """-> (statuses, one uint8 array per image); every output inside one 0xEE-filled tensor"""
    import torch
    from zlibstream_amd import png_decode_batch_device
    d_in = [_cuda(z) for z in streams]
    sizes = [h * ((w * b + 7) // 8) for (w, h), b in zip(shapes, bits)]
    d_out = [torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") for n in sizes]
    torch.cuda.synchronize()  # torch filled them on its own stream; the engine's stream does not wait for that one
    st = png_decode_batch_device(engine, [t.data_ptr() for t in d_in], [len(z) for z in streams], [w for w, _ in shapes], [h for _, h in shapes],
                                 list(bits), list(interlace), [t.data_ptr() for t in d_out], stream=stream)
    return st, [t.cpu().numpy() for t in d_out]


# ---------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def edge_images():
    """per bit depth: the pixel arrays of SHAPES and their raw scanline bytes, made once"""
    rng = np.random.default_rng(8020)
    out = {}
    for bits in BITS:
        px = [_random_px(rng, w, h, bits) for w, h in SHAPES]
        out[bits] = (px, [_pack(p, bits).tobytes() for p in px])
    return out


@pytest.mark.parametrize("bits", BITS)
def test_every_depth_at_the_edges(engine, edge_images, bits):
    rng = np.random.default_rng(100 + bits)
    px, raw = edge_images[bits]
    streams = [zlib.compress(_payload(rng, p, bits, 1), 6) for p in px]
    st, got = _decode(engine, streams, SHAPES, [bits] * len(SHAPES), [1] * len(SHAPES))
    assert st == [ZS_OK] * len(SHAPES), engine.last_error()
    for shape, g, want in zip(SHAPES, got, raw):
        assert g.tobytes() == want, (shape, bits)


@pytest.mark.parametrize("bits", BITS)
def test_merge_alone_on_random_pass_bytes(engine, bits):
    """zs_png_adam7_merge_batch_device fed random bytes, the padding bits of the pass rows included: what the restatement places,
    and zero padding bits in the image"""
    import torch
    from zlibstream_amd import png_adam7_merge_batch_device, png_idat_layout
    rng = np.random.default_rng(200 + bits)
    blobs, want = [], []
    for w, h in SHAPES:
        _, rb7, rows7 = png_idat_layout(w, h, bits, 1)
        blob = rng.integers(0, 256, sum(b * r for b, r in zip(rb7, rows7)), dtype=np.uint8)
        img = np.zeros((h, w) if bits < 8 else (h, w, bits // 8), dtype=np.uint8)
        at = 0
        for (xs, ys, xst, yst), rb, rows in zip(ADAM7, rb7, rows7):
            if rows == 0:
                continue
            pw = len(range(xs, w, xst))
            img[ys::yst, xs::xst] = _unpack(blob[at:at + rb * rows].reshape(rows, rb), pw, bits)
            at += rb * rows
        assert at == len(blob)
        blobs.append(blob)
        want.append(_pack(img, bits).tobytes())
    d_in = [_cuda(b.tobytes()) for b in blobs]
    d_out = [torch.full((len(x),), 0xEE, dtype=torch.uint8, device="cuda") for x in want]
    torch.cuda.synchronize()
    png_adam7_merge_batch_device(engine, [t.data_ptr() for t in d_in], [w for w, _ in SHAPES], [h for _, h in SHAPES], [bits] * len(SHAPES),
                                 [t.data_ptr() for t in d_out])
    for shape, t, x in zip(SHAPES, d_out, want):
        assert t.cpu().numpy().tobytes() == x, (shape, bits)


def test_non_interlaced_equals_the_two_existing_calls(engine):
    """a mixed batch, streams from the engine's own deflate_batch: the decode call, inflate_batch_device followed by
    png_unfilter_batch_device, and the pixels are the same bytes"""
    import torch
    from zlibstream_amd import png_unfilter_batch_device
    rng = np.random.default_rng(31)
    cases = [(1, 13, 6), (1, 16, 1), (8, 7, 5), (8, 64, 1), (24, 5, 9), (24, 21, 1), (64, 3, 4), (64, 9, 1), (1, 1, 1)]  # bits, width, height
    shapes = [(w, h) for _, w, h in cases]
    bits = [b for b, _, _ in cases]
    px = [_random_px(rng, w, h, b) for b, w, h in cases]
    raw = [_pack(p, b).tobytes() for p, b in zip(px, bits)]
    payloads = [_payload(rng, p, b, 0) for p, b in zip(px, bits)]
    streams = engine.deflate_batch(payloads, level=6)
    st, got = _decode(engine, streams, shapes, bits, [0] * len(cases))
    assert st == [ZS_OK] * len(cases), engine.last_error()
    d_in = [_cuda(z) for z in streams]
    d_mid = [torch.zeros(len(p), dtype=torch.uint8, device="cuda") for p in payloads]
    d_out = [torch.full((len(x),), 0xEE, dtype=torch.uint8, device="cuda") for x in raw]
    torch.cuda.synchronize()
    lens = engine.inflate_batch_device([t.data_ptr() for t in d_in], [len(z) for z in streams], [t.data_ptr() for t in d_mid], [len(p) for p in payloads])
    assert lens == [len(p) for p in payloads]
    rbs = [(w * b + 7) // 8 for (w, h), b in zip(shapes, bits)]
    assert png_unfilter_batch_device(engine, [t.data_ptr() for t in d_mid], rbs, [h for _, h in shapes], [max(1, b // 8) for b in bits],
                                     [t.data_ptr() for t in d_out]) == [ZS_OK] * len(cases)
    for case, g, t, x in zip(cases, got, d_out, raw):
        assert g.tobytes() == t.cpu().numpy().tobytes() == x, case


def test_round_trip_in_hbm(engine):
    """png_idat_batch_device (level 6, adaptive filter, a Write per row) and back: 8 images of 64 x 48 RGBA"""
    import torch
    from zlibstream_amd import deflate_bound, png_decode_batch_device, png_idat_batch_device
    n, w, h = 8, 64, 48
    rng = np.random.default_rng(77)
    imgs = [(_smooth_px(w, h, 4) + rng.integers(0, 3 + i, (h, w, 4), dtype=np.uint8)).astype(np.uint8) for i in range(n)]
    d_px = [_cuda(im.tobytes()) for im in imgs]
    cap = deflate_bound(h * (4 * w + 1)) + 48 * h + 96
    d_z = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
    d_back = [torch.full((4 * w * h,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    lens = png_idat_batch_device(engine, [t.data_ptr() for t in d_px], [4 * w] * n, [h] * n, [4] * n, [5] * n, [t.data_ptr() for t in d_z], [cap] * n,
                                 rows_per_write=1, level=6)
    st = png_decode_batch_device(engine, [t.data_ptr() for t in d_z], lens, [w] * n, [h] * n, [32] * n, [0] * n, [t.data_ptr() for t in d_back])
    assert st == [ZS_OK] * n, engine.last_error()
    for i in range(n):
        assert d_back[i].cpu().numpy().tobytes() == imgs[i].tobytes(), i


def test_block_parallel_inflate_path(engine):
    """one 512 x 512 RGBA interlaced image of smooth data: a stream well over 1 KiB, which inflate decodes block-parallel"""
    rng = np.random.default_rng(5)
    px = _smooth_px(512, 512, 4)
    z = zlib.compress(_payload(rng, px, 32, 1), 6)
    assert len(z) > 8 * 1024
    st, got = _decode(engine, [z], [(512, 512)], [32], [1])
    assert st == [ZS_OK], engine.last_error()
    assert got[0].tobytes() == px.tobytes()


def _decode_raw(engine, ptrs, lens, widths, heights, bits, interlace, outs, status=None, stream=0):
    from zlibstream_amd import _native
    n = len(ptrs)
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    st = I32(*(status if status is not None else [7] * n))
    rc = _native.lib().zs_png_decode_batch_device(engine.handle, n, VP(*ptrs), I64(*lens), I64(*widths), I64(*heights), I32(*bits), I32(*interlace),
                                                  VP(*outs), st, ctypes.c_void_p(stream))
    return rc, list(st)


def test_bad_images_beside_good_ones(engine):
    import torch
    rng = np.random.default_rng(66)
    shapes = [(33, 31), (21, 9), (16, 16), (16, 16), (12, 10), (9, 9)]
    bits = [24, 8, 8, 8, 16, 8]
    interlace = [1, 0, 0, 1, 0, 1]
    px = [_random_px(rng, w, h, b) for (w, h), b in zip(shapes, bits)]
    payloads = [_payload(rng, p, b, il) for p, b, il in zip(px, bits, interlace)]
    # image 4: one row short -- a valid stream of the wrong length
    payloads[4] = payloads[4][:-(12 * 2 + 1)]
    # image 5: filter type 5 on the only row of pass 3 of a 9 x 9 image (behind passes 1 and 2: 2 rows of 1 + 2 and 2 of 1 + 1 bytes)
    p5 = bytearray(payloads[5])
    assert p5[10] <= 4
    p5[10] = 5
    payloads[5] = bytes(p5)
    streams = [zlib.compress(p, 6) for p in payloads]
    streams[2] = streams[2][:-1] + bytes([streams[2][-1] ^ 0x55])  # a broken Adler-32
    streams[3] = streams[3][:-5]  # truncated
    d_in = [_cuda(z) for z in streams]
    sizes = [h * ((w * b + 7) // 8) for (w, h), b in zip(shapes, bits)]
    d_out = [torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") for n in sizes]
    torch.cuda.synchronize()
    rc, st = _decode_raw(engine, [t.data_ptr() for t in d_in], [len(z) for z in streams], [w for w, _ in shapes], [h for _, h in shapes], bits, interlace,
                         [t.data_ptr() for t in d_out])
    assert st == [0, 0, -3, -3, -3, -3]
    assert rc == ZS_DATA_ERROR
    assert "image 2" in engine.last_error() and "incorrect data check" in engine.last_error(), engine.last_error()
    for i in (0, 1):
        assert d_out[i].cpu().numpy().tobytes() == _pack(px[i], bits[i]).tobytes(), i
    # each failure alone names its image, and what is wrong with it
    for i, words in ((3, ("image 0",)), (4, ("image 0", "IDAT holds", "needs")), (5, ("image 0", "pass 3", "row 0"))):
        rc, st = _decode_raw(engine, [d_in[i].data_ptr()], [len(streams[i])], [shapes[i][0]], [shapes[i][1]], [bits[i]], [interlace[i]], [d_out[i].data_ptr()])
        assert (rc, st) == (ZS_DATA_ERROR, [ZS_DATA_ERROR])
        for word in words:
            assert word in engine.last_error(), (i, engine.last_error())


def test_nothing_is_written_outside_the_images(engine):
    """every out[i] a slice of one 0xEE-filled tensor at an odd byte offset: the bytes in front of and behind every image stay"""
    import torch
    from zlibstream_amd import png_decode_batch_device
    rng = np.random.default_rng(909)
    cases = [(bits, w, h, il) for bits in (1, 4, 24) for w, h in ((9, 9), (13, 6)) for il in (1, 0)]
    px = [_random_px(rng, w, h, b) for b, w, h, _ in cases]
    raw = [_pack(p, b).tobytes() for p, (b, _, _, _) in zip(px, cases)]
    streams = [zlib.compress(_payload(rng, p, b, il), 6) for p, (b, _, _, il) in zip(px, cases)]
    want = np.full(64 + sum(len(r) + 38 for r in raw), 0xEE, dtype=np.uint8)
    offs, at = [], 33
    for r in raw:
        offs.append(at)
        want[at:at + len(r)] = np.frombuffer(r, dtype=np.uint8)
        at += len(r) + 37
        at += 1 - at % 2  # odd
    assert all(o % 2 == 1 for o in offs) and at <= len(want)
    d_in = [_cuda(z) for z in streams]
    d_all = torch.full((len(want),), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = png_decode_batch_device(engine, [t.data_ptr() for t in d_in], [len(z) for z in streams], [w for _, w, _, _ in cases], [h for _, _, h, _ in cases],
                                 [b for b, _, _, _ in cases], [il for _, _, _, il in cases], [d_all.data_ptr() + o for o in offs])
    assert st == [ZS_OK] * len(cases), engine.last_error()
    got = d_all.cpu().numpy()
    for case, o, r in zip(cases, offs, raw):
        assert got[o:o + len(r)].tobytes() == r, case
    assert got.tobytes() == want.tobytes()


def test_on_the_callers_stream_and_live_argument_checks(engine):
    import torch
    rng = np.random.default_rng(404)
    shapes, bits, interlace = [(65, 33), (40, 12)], [32, 4], [1, 0]
    px = [_random_px(rng, w, h, b) for (w, h), b in zip(shapes, bits)]
    streams = [zlib.compress(_payload(rng, p, b, il), 6) for p, b, il in zip(px, bits, interlace)]
    host = [torch.from_numpy(np.frombuffer(z, dtype=np.uint8).copy()).pin_memory() for z in streams]
    d_in = [torch.zeros(len(z), dtype=torch.uint8, device="cuda") for z in streams]
    d_out = [torch.full((h * ((w * b + 7) // 8),), 0xEE, dtype=torch.uint8, device="cuda") for (w, h), b in zip(shapes, bits)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        scratch = torch.ones((1024, 1024), device="cuda")
        for _ in range(8):
            scratch = scratch @ scratch * 1e-3  # keeps the stream busy ahead of the fill of the input
        for d, hst in zip(d_in, host):
            d.copy_(hst, non_blocking=True)
        rc, st = _decode_raw(engine, [t.data_ptr() for t in d_in], [len(z) for z in streams], [w for w, _ in shapes], [h for _, h in shapes], bits, interlace,
                             [t.data_ptr() for t in d_out], stream=s.cuda_stream)
        got = [t.cpu().numpy().tobytes() for t in d_out]  # (the call has waited for the stream)
    assert (rc, st) == (ZS_OK, [0, 0]), engine.last_error()
    assert got == [_pack(p, b).tobytes() for p, b in zip(px, bits)]
    # bad arguments with a live context: ZS_STREAM_ERROR for the whole call, the statuses as they were
    good = dict(ptrs=[d_in[0].data_ptr()], lens=[len(streams[0])], widths=[65], heights=[33], bits=[32], interlace=[1], outs=[d_out[0].data_ptr()])
    for key, value in (("ptrs", [None]), ("outs", [None]), ("widths", [0]), ("heights", [0]), ("heights", [-2]), ("bits", [12]), ("bits", [0]),
                       ("interlace", [2]), ("interlace", [-1]), ("lens", [-1]), ("heights", [1 << 31])):
        assert _decode_raw(engine, **dict(good, **{key: value})) == (ZS_STREAM_ERROR, [7]), (key, value)
    from zlibstream_amd import _native
    L, h = _native.lib(), engine.handle
    assert L.zs_png_decode_batch_device(h, -1, None, None, None, None, None, None, None, None, None) == ZS_STREAM_ERROR
    assert L.zs_png_decode_batch_device(h, 1, None, None, None, None, None, None, None, None, None) == ZS_STREAM_ERROR
    assert L.zs_png_decode_batch_device(h, 0, None, None, None, None, None, None, None, None, None) == ZS_OK
    assert L.zs_png_adam7_merge_batch_device(h, 0, None, None, None, None, None, None) == ZS_OK
    assert L.zs_png_adam7_merge_batch_device(h, 1, None, None, None, None, None, None) == ZS_STREAM_ERROR
    # more than 2^31 - 1 rows, pass rows counted: three interlaced images 2 pixels wide have 3 pass rows for every 2 of their own
    # (3.15e9 for 2.1e9, payloads of 2.1e9 bytes each: inside what one stream may hold) -- refused before any device work
    big = {k: v * 3 for k, v in dict(good, widths=[2], heights=[700_000_000], bits=[1]).items()}
    assert _decode_raw(engine, **big) == (ZS_STREAM_ERROR, [7, 7, 7])
    assert "rows" in engine.last_error()
