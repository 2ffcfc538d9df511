"""Raw PNG scanlines to RGBA on the device (zs_png_expand_batch_device, KX) and whole files to RGBA
(zs_png_decode_files_rgba_batch).  The reference is a numpy restatement of the rules in include/zsgpu.h: np.unpackbits for the
low depths, integer scaling with divisions, a table lookup for palettes; every comparison is exact.  Pillow, where installed,
writes 8-bit files whose conversion to RGBA is the same by definition."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZS_OK, ZS_STREAM_ERROR, ZS_DATA_ERROR, ZS_BUF_ERROR = 0, -2, -3, -5
RGBA8, RGBA16 = 0, 1
SIG = b"\x89PNG\r\n\x1a\n"
SHAPES = ((1, 1), (3, 5), (33, 31), (257, 5), (1000, 3))
# PNG specification table 11.1
LEGAL = [(c, d) for c, ds in ((0, (1, 2, 4, 8, 16)), (2, (8, 16)), (3, (1, 2, 4, 8)), (4, (8, 16)), (6, (8, 16))) for d in ds]
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))  # xstart, ystart, xstep, ystep
GUARD = 64


# ---------------------------------------------------------------- the rules, restated
def _row_bytes(w, bits):
    return (w * bits + 7) // 8


def _samples(rows, w, color, depth):
    """(h, row_bytes) raw scanlines -> (h, w, channels) samples at their original depth"""
    h, ch = rows.shape[0], CHANNELS[color]
    if depth == 16:
        b = rows.reshape(h, w, ch, 2).astype(np.int64)
        return b[..., 0] * 256 + b[..., 1]
    if depth == 8:
        return rows.reshape(h, w, ch).astype(np.int64)
    b = np.unpackbits(rows, axis=1)[:, :w * depth].reshape(h, w, depth).astype(np.int64)
    return (b * (1 << np.arange(depth - 1, -1, -1))).sum(axis=2)[..., None]


def _scale(v, depth, target):
    if depth == target:
        return v
    if depth < target:
        return v * ((1 << target) - 1) // ((1 << depth) - 1)
    return (v * 255 + 32895) >> 16


def expand_ref(rows, w, color, depth, plte, trns, fmt):
    """-> the bytes of the expanded image: h rows of w * 4 uint8 or uint16 (little-endian), R, G, B, A"""
    target = 16 if fmt == RGBA16 else 8
    top = (1 << target) - 1
    s = _samples(rows, w, color, depth)
    h = s.shape[0]
    if color == 3:
        table = np.zeros((256, 4), dtype=np.int64)
        table[:, 3] = 255
        n = len(plte) // 3
        table[:n, :3] = np.frombuffer(plte, dtype=np.uint8).reshape(n, 3)
        table[:len(trns), 3] = np.frombuffer(trns, dtype=np.uint8)
        table[n:] = (0, 0, 0, 255)
        px = table[s[..., 0]] * (257 if target == 16 else 1)
    else:
        colors = 3 if color in (2, 6) else 1
        rgb = _scale(s[..., :colors], depth, target)
        if colors == 1:
            rgb = np.repeat(rgb, 3, axis=2)
        if color in (4, 6):
            a = _scale(s[..., colors], depth, target)
        elif trns:
            key = np.array([int.from_bytes(trns[2 * j:2 * j + 2], "big") % (1 << depth) for j in range(colors)], dtype=np.int64)
            a = np.where((s[..., :colors] == key).all(axis=2), 0, top)
        else:
            a = np.full((h, w), top, dtype=np.int64)
        px = np.concatenate([rgb, a[..., None]], axis=2)
    assert px.shape == (h, w, 4) and px.min() >= 0 and px.max() <= top
    return px.astype("<u2" if target == 16 else np.uint8).tobytes()


def make_image(rng, w, h, color, depth, with_trns, entries=None, trns_len=None):
    """random pixels (the padding bits of a row random too); a tRNS on request where the type has one: a key taken from a
    pixel and planted on others, with bits above the depth set in the chunk; a palette of `entries` entries"""
    bits = depth * CHANNELS[color]
    rows = rng.integers(0, 256, (h, _row_bytes(w, bits)), dtype=np.uint8)
    plte = trns = b""
    if color == 3:
        entries = entries or min(256, (1 << depth))
        plte = bytes(rng.integers(0, 256, 3 * entries, dtype=np.uint8))
        if with_trns:
            trns = bytes(rng.integers(0, 256, trns_len or (entries + 1) // 2, dtype=np.uint8))
    elif with_trns and color in (0, 2):
        if depth >= 8:
            bpp = bits // 8
            px = rows.reshape(h, w, bpp)
            key = px[rng.integers(0, h), rng.integers(0, w)].copy()
            plant = rng.random((h, w)) < 0.2
            px[plant] = key
            near = rng.random((h, w)) < 0.1  # the key but for one bit of its first byte: not the key
            px[near] = key ^ np.eye(1, bpp, 0, dtype=np.uint8)[0]
            ks = key.reshape(-1, depth // 8)
            trns = b"".join(bytes(k) if depth == 16 else bytes([int(rng.integers(0, 256)), int(k[0])]) for k in ks)
        else:
            trns = struct.pack(">H", int(rng.integers(0, 1 << 16)))  # (of 2, 4 or 16 values: random pixels meet it)
    return dict(w=w, h=h, color=color, depth=depth, rows=rows, plte=plte, trns=trns)


# ---------------------------------------------------------------- device plumbing
def _cuda(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def _px(fmt):
    return 8 if fmt == RGBA16 else 4


def run_expand(engine, imgs, fmt, stream=None):
    """one call over imgs -> the expanded bytes per image; every output in a 0xEE-filled tensor of its own with GUARD bytes in
    front of it and behind it, both checked"""
    import torch
    from zlibstream_amd import png_expand_batch_device
    d_in = [_cuda(im["rows"].tobytes()) for im in imgs]
    sizes = [im["w"] * im["h"] * _px(fmt) for im in imgs]
    d_out = [torch.full((GUARD + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for n in sizes]
    torch.cuda.synchronize()  # torch filled them on its own stream; the engine's stream does not wait for that one
    png_expand_batch_device(engine, [t.data_ptr() for t in d_in], [im["w"] for im in imgs], [im["h"] for im in imgs], [im["depth"] for im in imgs],
                            [im["color"] for im in imgs], [t.data_ptr() + GUARD for t in d_out], plte=[im["plte"] or None for im in imgs],
                            trns=[im["trns"] or None for im in imgs], format=fmt, stream=stream)
    if stream is not None:
        torch.cuda.synchronize()
    got = []
    for t, n in zip(d_out, sizes):
        b = t.cpu().numpy().tobytes()
        assert b[:GUARD] == b"\xEE" * GUARD and b[GUARD + n:] == b"\xEE" * GUARD, "bytes outside an output were written"
        got.append(b[GUARD:GUARD + n])
    return got


def want_of(im, fmt):
    return expand_ref(im["rows"], im["w"], im["color"], im["depth"], im["plte"], im["trns"], fmt)


@pytest.fixture(scope="module")
def images():
    """(color, depth) -> one image per shape of SHAPES, a tRNS on every other one where the type has one; made once"""
    rng = np.random.default_rng(8101)
    return {(c, d): [make_image(rng, w, h, c, d, with_trns=k % 2 == 0) for k, (w, h) in enumerate(SHAPES)] for c, d in LEGAL}


# ---------------------------------------------------------------- the expansion
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
@pytest.mark.parametrize("color,depth", LEGAL)
def test_every_legal_pair(engine, images, color, depth, fmt):
    imgs = images[color, depth]
    if color in (0, 2, 3):
        assert [bool(im["trns"]) for im in imgs] == [True, False, True, False, True]
    got = run_expand(engine, imgs, fmt)
    for im, g in zip(imgs, got):
        assert g == want_of(im, fmt), (im["w"], im["h"])
    if color in (0, 2):  # the keys bite, and not everywhere
        alpha = np.frombuffer(got[4], dtype=np.uint8).reshape(-1, _px(fmt))[:, -1]
        assert 0 < np.count_nonzero(alpha == 0) < alpha.size


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_a_mixed_batch_at_every_alignment(engine, fmt):
    """all fifteen pairs in one call, every image another shape, the outputs carved from one buffer at every legal residue
    modulo 16: the same bytes as fifteen single calls and as the restatement, and nothing written between the outputs"""
    import torch
    from zlibstream_amd import png_expand_batch_device
    rng = np.random.default_rng(8102 + fmt)
    px = _px(fmt)
    imgs = [make_image(rng, 5 + 23 * k, 1 + (7 * k) % 11, c, d, with_trns=k % 3 != 1) for k, (c, d) in enumerate(LEGAL)]
    offs, at = [], 0
    for k, im in enumerate(imgs):
        at = (at + GUARD + 15) // 16 * 16 + (k * px) % 16  # residues 0, 4, 8, 12 (RGBA8) or 0, 8 (RGBA16) in turn
        offs.append(at)
        at += im["w"] * im["h"] * px
    assert {o % 16 for o in offs} == set(range(0, 16, px))
    buf = torch.full((at + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    d_in = [_cuda(im["rows"].tobytes()) for im in imgs]
    torch.cuda.synchronize()
    png_expand_batch_device(engine, [t.data_ptr() for t in d_in], [im["w"] for im in imgs], [im["h"] for im in imgs], [im["depth"] for im in imgs],
                            [im["color"] for im in imgs], [buf.data_ptr() + o for o in offs], plte=[im["plte"] or None for im in imgs],
                            trns=[im["trns"] or None for im in imgs], format=fmt)
    b = buf.cpu().numpy().tobytes()
    at = 0
    for im, o in zip(imgs, offs):
        n = im["w"] * im["h"] * px
        assert b[at:o] == b"\xEE" * (o - at), "bytes between two outputs were written"
        want = want_of(im, fmt)
        assert b[o:o + n] == want, (im["color"], im["depth"])
        assert run_expand(engine, [im], fmt)[0] == want
        at = o + n
    assert b[at:] == b"\xEE" * GUARD


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_palette_edges(engine, fmt):
    """palettes of 1 and of 256 entries; at 1, 2 and 4 bits palettes shorter than 2^depth with indexes beyond them (opaque
    black); a tRNS shorter than its PLTE (the entries past it opaque) and one as long as it"""
    rng = np.random.default_rng(8103)
    imgs = [make_image(rng, 67, 9, 3, 8, False, entries=1), make_image(rng, 67, 9, 3, 8, True, entries=1, trns_len=1),
            make_image(rng, 130, 4, 3, 8, False, entries=256), make_image(rng, 130, 4, 3, 8, True, entries=256, trns_len=256),
            make_image(rng, 130, 4, 3, 8, True, entries=256, trns_len=3), make_image(rng, 131, 3, 3, 1, True, entries=1, trns_len=1),
            make_image(rng, 131, 3, 3, 2, True, entries=3, trns_len=2), make_image(rng, 131, 3, 3, 4, True, entries=5, trns_len=1),
            make_image(rng, 131, 3, 3, 4, False, entries=15), make_image(rng, 77, 2, 3, 8, True, entries=200, trns_len=199)]
    got = run_expand(engine, imgs, fmt)
    for im, g in zip(imgs, got):
        assert g == want_of(im, fmt), (im["depth"], len(im["plte"]) // 3, len(im["trns"]))
    # the restatement itself, on the points this test is about
    one = np.frombuffer(got[0], dtype=np.uint8 if fmt == RGBA8 else "<u2").reshape(-1, 4)
    idx = imgs[0]["rows"].reshape(-1)
    m = 257 if fmt == RGBA16 else 1
    assert (one[idx != 0] == (0, 0, 0, 255 * m)).all() and (one[idx == 0] == tuple(v * m for v in imgs[0]["plte"]) + (255 * m,)).all()
    short = np.frombuffer(got[4], dtype=np.uint8 if fmt == RGBA8 else "<u2").reshape(-1, 4)
    idx = imgs[4]["rows"].reshape(-1)
    assert (short[idx >= 3, 3] == 255 * m).all() and (short[idx == 1, 3] == imgs[4]["trns"][1] * m).all()


def test_a_stream_of_the_caller_and_an_empty_call(engine, images):
    import torch
    from zlibstream_amd import png_expand_batch_device
    s = torch.cuda.Stream()
    imgs = [images[6, 16][3], images[3, 2][4], images[0, 4][2]]
    got = run_expand(engine, imgs, RGBA8, stream=s.cuda_stream)
    assert got == [want_of(im, RGBA8) for im in imgs]
    assert png_expand_batch_device(engine, [], [], [], [], [], []) is None


def test_bad_arguments_are_stream_errors_and_touch_nothing(engine):
    from zlibstream_amd import _native
    L = _native.lib()
    rows = np.arange(12, dtype=np.uint8)
    d_in, d_out = _cuda(rows.tobytes()), _cuda(b"\xEE" * 4096)
    VP, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    plte, trns = bytes(range(30)), bytes(range(6))
    p_plte, p_trns = ctypes.cast(ctypes.c_char_p(plte), VP).value, ctypes.cast(ctypes.c_char_p(trns), VP).value

    def call(n=1, ctx=engine.handle, inp=(d_in.data_ptr(),), w=(3,), h=(4,), depth=(8,), color=(0,), pl=(p_plte,), ent=(10,), tr=(p_trns,), tl=(0,),
             fmt=RGBA8, out=(d_out.data_ptr(),)):
        arr = lambda t, v: None if v is None else (t * len(v))(*v)
        return L.zs_png_expand_batch_device(ctx, n, arr(VP, inp), arr(I64, w), arr(I64, h), arr(I32, depth), arr(I32, color), arr(VP, pl), arr(I32, ent),
                                            arr(VP, tr), arr(I32, tl), fmt, arr(VP, out), None)

    bad = [dict(ctx=None), dict(n=-1), dict(inp=None), dict(w=None), dict(h=None), dict(depth=None), dict(color=None), dict(out=None),
           dict(inp=(None,)), dict(out=(None,)),
           dict(color=(2,), depth=(4,)), dict(color=(3,), depth=(16,)), dict(color=(5,)), dict(color=(4,), depth=(2,)), dict(color=(6,), depth=(4,)), dict(depth=(3,)),
           dict(depth=(0,)), dict(w=(0,)), dict(w=(1 << 31,)), dict(h=(0,)), dict(h=(1 << 31,)), dict(w=(-1,)),
           dict(color=(3,), pl=None), dict(color=(3,), pl=(None,)), dict(color=(3,), ent=None), dict(color=(3,), ent=(0,)), dict(color=(3,), ent=(257,)),
           dict(color=(3,), tl=(11,)), dict(color=(3,), tl=(-1,)), dict(color=(3,), tl=(2,), tr=None), dict(color=(3,), tl=(2,), tr=(None,)),
           dict(tl=(1,)), dict(tl=(3,)), dict(tl=(6,)), dict(tl=(2,), tr=None), dict(tl=(2,), tr=(None,)),
           dict(color=(2,), w=(1,), tl=(2,)), dict(color=(2,), w=(1,), tl=(5,)), dict(color=(2,), w=(1,), tl=(6,), tr=(None,)),
           dict(fmt=2), dict(fmt=-1), dict(out=(d_out.data_ptr() + 2,)), dict(out=(d_out.data_ptr() + 1,)), dict(fmt=RGBA16, out=(d_out.data_ptr() + 4,)),
           # more than 2^31 - 1 rows in one call: refused before anything is read
           dict(n=2, inp=(d_in.data_ptr(),) * 2, w=(1, 1), h=((1 << 31) - 1, 1), depth=(8, 8), color=(0, 0), pl=None, ent=None, tr=None, tl=None,
                out=(d_out.data_ptr(),) * 2)]
    for kw in bad:
        assert call(**kw) == ZS_STREAM_ERROR, kw
    assert call(n=0, inp=None, w=None, h=None, depth=None, color=None, pl=None, ent=None, tr=None, tl=None, out=None) == ZS_OK
    assert d_out.cpu().numpy().tobytes() == b"\xEE" * 4096
    # the same call with nothing wrong, the optional arrays absent, and the counts that are ignored at types 4 and 6 absurd
    assert call(pl=None, ent=None, tr=None, tl=None) == ZS_OK
    assert d_out.cpu().numpy()[:48].tobytes() == expand_ref(rows.reshape(4, 3), 3, 0, 8, b"", b"", RGBA8)
    assert call(color=(4,), w=(1,), h=(6,), pl=(None,), ent=(999,), tr=(None,), tl=(77,), fmt=RGBA16) == ZS_OK
    assert d_out.cpu().numpy()[:48].tobytes() == expand_ref(rows.reshape(6, 2), 1, 4, 8, b"", b"", RGBA16)


# ---------------------------------------------------------------- files
def chunk(ctype, data, crc=None):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data) if crc is None else crc)


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


def _filtered(rows, k):
    """filter types None and Up in turn (PNG specification 9.2): (h, rb) -> the bytes of h rows of 1 + rb"""
    types = (np.arange(rows.shape[0]) + k) % 2 * 2
    above = np.zeros_like(rows)
    above[1:] = rows[:-1]
    f = np.where(types[:, None] == 2, rows - above, rows)  # (uint8 wraps)
    return np.concatenate([types[:, None].astype(np.uint8), f], axis=1).tobytes()


def build_png(im, interlace, k=0, before=None, crc_flip=None):
    """a whole file around im's scanlines: PLTE and tRNS in front of the IDAT chunks (or `before` in their place), the
    stream stored or compressed and cut into two IDAT chunks"""
    w, h, depth, color = im["w"], im["h"], im["depth"], im["color"]
    bits = depth * CHANNELS[color]
    rows = im["rows"].copy()
    used = (w * bits) % 8
    if used:
        rows[:, -1] &= (0xFF00 >> used) & 0xFF  # (what a decoder leaves in the padding bits of an interlaced image is zero)
    if interlace:
        px, payload = _unpack(rows, w, bits), b""
        for xs, ys, xst, yst in ADAM7:
            sub = px[ys::yst, xs::xst]
            if sub.shape[0] and sub.shape[1]:
                payload += _filtered(_pack(sub, bits), k)
    else:
        payload = _filtered(rows, k)
    stream = zlib.compress(payload, 0 if k % 3 == 0 else 6)
    if before is None:
        before = ([chunk(b"PLTE", im["plte"])] if im["plte"] else []) + ([chunk(b"tRNS", im["trns"])] if im["trns"] else [])
    cut = len(stream) // 2
    f = (SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color, 0, 0, interlace)) + chunk(b"gAMA", struct.pack(">I", 45455)) + b"".join(before) +
         chunk(b"IDAT", stream[:cut]) + chunk(b"IDAT", stream[cut:]) + chunk(b"IEND", b""))
    return f, rows


@pytest.fixture(scope="module")
def files():
    """every legal pair, interlaced and not -> (files, images with the padding bits as a decoder leaves them)"""
    rng = np.random.default_rng(8104)
    out_f, out_im = [], []
    for k, (c, d) in enumerate(LEGAL):
        for interlace, (w, h) in ((0, (33, 31)), (1, (21, 13))):
            im = make_image(rng, w, h, c, d, with_trns=(k + interlace) % 2 == 0)
            f, rows = build_png(im, interlace, k=k + interlace)
            out_f.append(f), out_im.append(dict(im, rows=rows))
    return out_f, out_im


def decode_rgba(engine, batch, fmt, caps=None, stream=None):
    """-> (statuses, infos, one bytes object per file: GUARD, the output's capacity, GUARD)"""
    import torch
    from zlibstream_amd import png_decode_files_rgba_batch
    caps = caps or [1 << 16] * len(batch)
    d_out = [torch.full((GUARD + c + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for c in caps]
    torch.cuda.synchronize()
    st, infos = png_decode_files_rgba_batch(engine, batch, [t.data_ptr() + GUARD for t in d_out], caps, format=fmt, stream=stream)
    torch.cuda.synchronize()
    return st, infos, [t.cpu().numpy().tobytes() for t in d_out]


def _check_output(buf, want):
    assert buf[:GUARD] == b"\xEE" * GUARD, "bytes in front of an output were written"
    assert buf[GUARD:GUARD + len(want)] == want
    assert buf[GUARD + len(want):] == b"\xEE" * (len(buf) - GUARD - len(want)), "bytes behind an image were written"


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_files_to_rgba_every_pair_interlaced_and_not(engine, files, fmt):
    fs, ims = files
    caps = [im["w"] * im["h"] * _px(fmt) for im in ims]
    st, infos, got = decode_rgba(engine, fs, fmt, caps=caps)
    assert st == [ZS_OK] * len(fs), engine.last_error()
    for im, inf, g in zip(ims, infos, got):
        assert (inf["width"], inf["height"], inf["bit_depth"], inf["color_type"]) == (im["w"], im["h"], im["depth"], im["color"])
        _check_output(g, want_of(im, fmt))


def _flip(f, i):
    return f[:i] + bytes([f[i] ^ 0x04]) + f[i + 1:]


def _broken(files):
    """-> (batch, wanted status per file, the image behind every good file or None, a needle of the first failure's message)"""
    fs, ims = files
    by = {(im["color"], im["depth"], i % 2): i for i, im in enumerate(ims)}
    rng = np.random.default_rng(8105)
    pal = dict(ims[by[3, 8, 0]])
    no_plte, _ = build_png(pal, 0, before=[])
    gray = make_image(rng, 33, 31, 0, 8, True)
    long_trns, _ = build_png(gray, 0, before=[chunk(b"tRNS", gray["trns"] + b"\x00")])
    bad_crc, _ = build_png(gray, 0, before=[chunk(b"tRNS", gray["trns"], crc=zlib.crc32(b"tRNS" + gray["trns"]) ^ 1)])
    good = fs[by[2, 8, 0]]
    at = good.index(b"IDAT") + 4 + 20
    bad_idat = _flip(good, at)
    batch = [fs[by[6, 16, 1]], no_plte, fs[by[3, 4, 1]], long_trns, bad_crc, fs[by[0, 1, 0]], bad_idat, fs[by[4, 8, 0]], fs[by[2, 16, 1]]]
    want_st = [ZS_OK, ZS_DATA_ERROR, ZS_OK, ZS_DATA_ERROR, ZS_DATA_ERROR, ZS_OK, ZS_DATA_ERROR, ZS_OK, ZS_OK]
    src = [ims[by[6, 16, 1]], None, ims[by[3, 4, 1]], None, None, ims[by[0, 1, 0]], None, ims[by[4, 8, 0]], ims[by[2, 16, 1]]]
    return batch, want_st, src, bad_crc


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_a_file_fails_for_itself_only(engine, files, fmt):
    batch, want_st, src, _ = _broken(files)
    caps = [1 << 16] * len(batch)
    caps[7] = src[7]["w"] * src[7]["h"] * _px(fmt) - 1  # one byte short: nothing is written for that file
    want_st = list(want_st)
    want_st[7] = ZS_BUF_ERROR
    st, infos, got = decode_rgba(engine, batch, fmt, caps=caps)
    assert st == want_st, engine.last_error()
    # the first failing file is the palette file without a PLTE
    assert engine.last_error().startswith("data error: file 1: ") and "PLTE" in engine.last_error(), engine.last_error()
    for j, im in enumerate(src):
        if want_st[j] == ZS_OK:
            _check_output(got[j], want_of(im, fmt))
    assert got[7] == b"\xEE" * len(got[7])
    # one by one, every failure names itself
    for j, needle in ((3, "tRNS holds 3 bytes"), (4, "CRC error in tRNS chunk"), (6, "CRC error in IDAT chunk")):
        st, _, _ = decode_rgba(engine, [batch[0], batch[j]], fmt)
        assert st == [ZS_OK, ZS_DATA_ERROR] and engine.last_error().startswith("data error: file 1: ") and needle in engine.last_error(), engine.last_error()
    st, _, _ = decode_rgba(engine, [batch[0], batch[7]], fmt, caps=[1 << 16, caps[7]])
    assert st == [ZS_OK, ZS_BUF_ERROR] and engine.last_error().startswith("buffer error: file 1: "), engine.last_error()


def test_the_raw_decode_call_is_unchanged(engine, files):
    """on the same files zs_png_decode_files_batch still gives the raw scanlines, and still interprets no ancillary chunk: the
    tRNS with a wrong CRC or a wrong length and the palette file without a PLTE decode"""
    import torch
    from zlibstream_amd import png_decode_files_batch
    fs, ims = files
    batch, want_st, src, bad_crc = _broken(files)
    rng = np.random.default_rng(8105)
    gray = make_image(rng, 33, 31, 0, 8, True)  # (the image _broken made: the same seed)
    assert build_png(gray, 0, before=[chunk(b"tRNS", gray["trns"], crc=zlib.crc32(b"tRNS" + gray["trns"]) ^ 1)])[0] == bad_crc
    all_f = list(fs) + [batch[1], batch[3], batch[4]]
    all_rows = [im["rows"] for im in ims] + [src_rows for src_rows in (ims[[i for i, im in enumerate(ims) if (im["color"], im["depth"]) == (3, 8)][0]]["rows"],
                                                                       gray["rows"], gray["rows"])]
    d_out = [torch.full((r.size + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for r in all_rows]
    torch.cuda.synchronize()
    st, infos = png_decode_files_batch(engine, all_f, [t.data_ptr() for t in d_out], [r.size for r in all_rows])
    assert st == [ZS_OK] * len(all_f), engine.last_error()
    for t, r in zip(d_out, all_rows):
        b = t.cpu().numpy().tobytes()
        assert b[:r.size] == r.tobytes() and b[r.size:] == b"\xEE" * GUARD


def test_files_bad_arguments(engine, files):
    from zlibstream_amd import _native
    L = _native.lib()
    f = files[0][0]
    d_out = _cuda(b"\xEE" * 8192)
    VP, I64, I32 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_int * 1
    fp = VP(ctypes.cast(ctypes.c_char_p(f), ctypes.c_void_p).value)
    o, n, cap = VP(d_out.data_ptr()), I64(len(f)), I64(8192)
    for a in ((-1, fp, n, RGBA8, o, cap), (1, None, n, RGBA8, o, cap), (1, fp, None, RGBA8, o, cap), (1, fp, n, RGBA8, None, cap), (1, fp, n, RGBA8, o, None),
              (1, VP(None), n, RGBA8, o, cap), (1, fp, I64(-1), RGBA8, o, cap), (1, fp, n, RGBA8, VP(None), cap), (1, fp, n, RGBA8, o, I64(-1)),
              (1, fp, n, 2, o, cap), (1, fp, n, -1, o, cap), (1, fp, n, RGBA8, VP(d_out.data_ptr() + 2), cap), (1, fp, n, RGBA16, VP(d_out.data_ptr() + 4), cap)):
        st = I32(77)
        assert L.zs_png_decode_files_rgba_batch(engine.handle, a[0], a[1], a[2], a[3], a[4], a[5], None, st, None) == ZS_STREAM_ERROR and st[0] == 77, a
    assert L.zs_png_decode_files_rgba_batch(None, 1, fp, n, RGBA8, o, cap, None, None, None) == ZS_STREAM_ERROR
    assert L.zs_png_decode_files_rgba_batch(engine.handle, 0, None, None, RGBA8, None, None, None, None, None) == ZS_OK
    assert d_out.cpu().numpy().tobytes() == b"\xEE" * 8192


def test_the_stage_timer_shows_the_expansion(engine, images, files):
    engine.set_profiling(True)
    try:
        got = run_expand(engine, images[2, 8][2:4], RGBA16)
        alone = engine.stage_ms()
        st, _, _ = decode_rgba(engine, files[0][:4], RGBA8)
        whole = engine.stage_ms()
    finally:
        engine.set_profiling(False)
    assert got == [want_of(im, RGBA16) for im in images[2, 8][2:4]] and st == [ZS_OK] * 4
    assert alone.get("png_expand", 0) > 0, alone
    assert whole.get("png_expand", 0) > 0 and whole.get("crc32_frame", 0) > 0, whole


# ---------------------------------------------------------------- Pillow
def test_rgba_of_what_pil_saves(engine):
    """8-bit files of modes P (with and without transparency), L, LA, RGB and RGBA: Pillow's convert("RGBA") is the rules of
    this expansion there (not at 16 bits or for gray below 8 bits, where its conversions differ)."""
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    rng = np.random.default_rng(8106)
    w, h = 203, 57
    y, x = np.mgrid[0:h, 0:w]
    made = []
    for mode, nb in (("L", 1), ("LA", 2), ("RGB", 3), ("RGBA", 4)):
        a = np.stack([((x * (c + 2) + y * 3 + rng.integers(0, 4, x.shape)) & 255) for c in range(nb)], axis=2).astype(np.uint8)
        made.append((Image.frombytes(mode, (w, h), a.tobytes()), {}))
    for colors, transparency in ((256, None), (256, bytes(rng.integers(0, 256, 256, dtype=np.uint8))), (200, bytes(rng.integers(0, 256, 77, dtype=np.uint8))),
                                 (256, 9), (13, bytes([0, 128, 255])), (2, None)):
        a = rng.integers(0, colors, (h, w), dtype=np.uint8)
        im = Image.frombytes("P", (w, h), a.tobytes())
        im.putpalette(bytes(rng.integers(0, 256, 3 * colors, dtype=np.uint8)))
        made.append((im, {} if transparency is None else {"transparency": transparency}))
    batch, want = [], []
    for im, kw in made:
        b = io.BytesIO()
        im.save(b, "PNG", **kw)
        batch.append(b.getvalue())
        back = Image.open(io.BytesIO(b.getvalue()))
        want.append(back.convert("RGBA").tobytes())
    st, infos, got = decode_rgba(engine, batch, RGBA8, caps=[w * h * 4] * len(batch))
    assert st == [ZS_OK] * len(batch), engine.last_error()
    assert {i["color_type"] for i in infos} == {0, 2, 3, 4, 6} and len({i["bit_depth"] for i in infos if i["color_type"] == 3}) > 1, infos
    for k, (g, wnt) in enumerate(zip(got, want)):
        assert g[GUARD:GUARD + w * h * 4] == wnt, (k, infos[k])
