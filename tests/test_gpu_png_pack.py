"""RGBA pixels to raw PNG scanlines on the device (zs_png_pack_batch_device, KG), the inverse of the expansion (KX).  The
references are numpy restatements of the rules in include/zsgpu.h, written here: expand_ref (np.unpackbits, integer scaling
with divisions, a table lookup) and pack_ref (divisions, a palette searched entry by entry, np.packbits); every comparison is
exact."""
import ctypes
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZS_OK, ZS_STREAM_ERROR = 0, -2
RGBA8, RGBA16 = 0, 1
SHAPES = ((1, 1), (3, 5), (33, 31), (257, 5), (1000, 3))
# PNG specification table 11.1
LEGAL = [(c, d) for c, ds in ((0, (1, 2, 4, 8, 16)), (2, (8, 16)), (3, (1, 2, 4, 8)), (4, (8, 16)), (6, (8, 16))) for d in ds]
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
GUARD = 64


# ---------------------------------------------------------------- the rules, restated
def _row_bytes(w, bits):
    return (w * bits + 7) // 8


def _px(fmt):
    return 8 if fmt == RGBA16 else 4


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


def _palette(plte, trns, n=None):
    """-> (n, 4) entries R, G, B, A: the first n of the PLTE's (all by default)"""
    n = len(plte) // 3 if n is None else min(n, len(plte) // 3)
    table = np.full((n, 4), 255, dtype=np.int64)
    table[:, :3] = np.frombuffer(plte, dtype=np.uint8).reshape(-1, 3)[:n]
    t = np.frombuffer(trns, dtype=np.uint8)[:n]
    table[:len(t), 3] = t
    return table


def expand_ref(rows, w, color, depth, plte, trns, fmt):
    """KX: raw scanlines -> (h, w, 4) int64 R, G, B, A at 8 or 16 bits"""
    target = 16 if fmt == RGBA16 else 8
    top = (1 << target) - 1
    s = _samples(rows, w, color, depth)
    h = s.shape[0]
    if color == 3:
        table = np.zeros((256, 4), dtype=np.int64)
        table[:, 3] = 255
        table[:len(plte) // 3] = _palette(plte, trns)
        return table[s[..., 0]] * (257 if target == 16 else 1)
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
    return np.concatenate([rgb, a[..., None]], axis=2)


def _reduce(v, fmt, depth):
    """a source sample of 8 or 16 bits to `depth` bits"""
    if fmt == RGBA8:
        return v * 257 if depth == 16 else v // (256 >> depth)
    if depth == 16:
        return v
    return ((v * 255 + 32895) // 65536) // (256 >> depth)


def pack_ref(px, color, depth, plte, trns, fmt):
    """KG: (h, w, 4) int64 pixels -> ((h, row_bytes) uint8 raw scanlines, pixels of a palette image without an entry)"""
    h, w, _ = px.shape
    miss = 0
    if color == 3:
        c8 = _reduce(px, fmt, 8)
        table = _palette(plte, trns, 1 << depth)  # (an entry at or beyond 2^depth has no index)
        eq = (c8[:, :, None, :] == table[None, None, :, :]).all(axis=3)
        found = eq.any(axis=2)
        s = np.where(found, eq.argmax(axis=2), 0)[..., None]  # (argmax: the first)
        miss = int(np.count_nonzero(~found))
    else:
        colors = 3 if color in (2, 6) else 1
        s = _reduce(px[..., :colors], fmt, depth)
        if color in (4, 6):
            s = np.concatenate([s, _reduce(px[..., 3:4], fmt, depth)], axis=2)
        elif trns:
            key = np.array([int.from_bytes(trns[2 * j:2 * j + 2], "big") % (1 << depth) for j in range(colors)], dtype=np.int64)
            s = np.where(px[..., 3:4] == 0, key, s)
    if depth == 16:
        rows = np.stack([s >> 8, s & 255], axis=-1).reshape(h, -1).astype(np.uint8)
    elif depth == 8:
        rows = s.reshape(h, -1).astype(np.uint8)
    else:
        bits = (s[..., 0][:, :, None] >> np.arange(depth - 1, -1, -1)) & 1
        rows = np.packbits(bits.reshape(h, w * depth).astype(np.uint8), axis=1)  # (the last byte's unused low bits: zero)
    assert rows.shape == (h, _row_bytes(w, depth * CHANNELS[color]))
    return rows, miss


def px_bytes(px, fmt):
    return px.astype("<u2" if fmt == RGBA16 else np.uint8).tobytes()


def distinct_palette(rng, entries):
    """`entries` colours that differ in R, G, B, any alpha -> (plte, trns); a palette a pack can invert, whatever part of the
    tRNS is kept"""
    c = rng.choice(1 << 24, size=entries, replace=False).astype(np.uint64)
    rgb = np.stack([(c >> s) & 255 for s in (0, 8, 16)], axis=1).astype(np.uint8)
    return rgb.tobytes(), bytes(rng.integers(0, 256, entries, dtype=np.uint8))


def make_raw(rng, w, h, color, depth, with_trns, fmt, representable=True):
    """random raw scanlines with the padding bits zero; palette indexes below the entry count, the palette's colours distinct;
    a tRNS key taken from a pixel and planted on others.  representable: at 16 bits for an RGBA8 target the samples are
    multiples of 257 -- the only ones that survive the way through 8 bits"""
    bits = depth * CHANNELS[color]
    rows = rng.integers(0, 256, (h, _row_bytes(w, bits)), dtype=np.uint8)
    plte = trns = b""
    if depth == 16 and fmt == RGBA8 and representable:
        rows[:, 1::2] = rows[:, 0::2]
    if color == 3:
        entries = int(rng.integers(1, (1 << depth) + 1)) if depth < 8 else (256 if w % 2 else 199)
        idx = rng.integers(0, entries, (h, w))
        rows = np.packbits(((idx[:, :, None] >> np.arange(depth - 1, -1, -1)) & 1).reshape(h, -1).astype(np.uint8), axis=1)
        plte, trns = distinct_palette(rng, entries)
        if not with_trns:
            trns = b""
        elif w % 3 == 0:
            trns = trns[:(entries + 1) // 2]
    elif with_trns and color in (0, 2):
        s = _samples(rows, w, color, depth)
        key = s[rng.integers(0, h), rng.integers(0, w)]
        s[rng.random((h, w)) < 0.2] = key
        if depth == 16:
            rows = np.stack([s >> 8, s & 255], axis=-1).reshape(h, -1).astype(np.uint8)
        elif depth == 8:
            rows = s.reshape(h, -1).astype(np.uint8)
        else:
            rows = np.packbits(((s[..., 0][:, :, None] >> np.arange(depth - 1, -1, -1)) & 1).reshape(h, -1).astype(np.uint8), axis=1)
        above = int(rng.integers(0, 1 << 16)) & ~((1 << depth) - 1) & 0xFFFF  # (bits above the depth do not count)
        trns = b"".join(struct.pack(">H", int(k) | above) for k in key)
    used = (w * bits) % 8
    if used:
        rows[:, -1] &= (0xFF00 >> used) & 0xFF
    return dict(w=w, h=h, color=color, depth=depth, rows=np.ascontiguousarray(rows), plte=plte, trns=trns)


# ---------------------------------------------------------------- device plumbing
def _cuda(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def run_pack(engine, imgs, pixels, fmt, stream=None, unmatched=True):
    """one call over imgs (pixels[i]: the RGBA bytes of image i) -> (the packed bytes per image, the unmatched counts); every
    output in a 0xEE-filled tensor of its own with GUARD bytes in front of it and behind it, both checked"""
    import torch
    from zlibstream_amd import png_pack_batch_device
    d_in = [_cuda(p) for p in pixels]
    sizes = [_row_bytes(im["w"], im["depth"] * CHANNELS[im["color"]]) * im["h"] for im in imgs]
    d_out = [torch.full((GUARD + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for n in sizes]
    torch.cuda.synchronize()  # torch filled them on its own stream; the engine's stream does not wait for that one
    counts = png_pack_batch_device(engine, [t.data_ptr() for t in d_in], [im["w"] for im in imgs], [im["h"] for im in imgs], [im["depth"] for im in imgs],
                                   [im["color"] for im in imgs], [t.data_ptr() + GUARD for t in d_out], plte=[im["plte"] or None for im in imgs],
                                   trns=[im["trns"] or None for im in imgs], format=fmt, stream=stream, return_unmatched=unmatched)
    if stream is not None:
        torch.cuda.synchronize()
    got = []
    for t, n in zip(d_out, sizes):
        b = t.cpu().numpy().tobytes()
        assert b[:GUARD] == b"\xEE" * GUARD and b[GUARD + n:] == b"\xEE" * GUARD, "bytes outside an output were written"
        got.append(b[GUARD:GUARD + n])
    return got, counts


def device_expand(engine, imgs, fmt):
    """png_expand_batch_device over imgs -> the RGBA bytes per image"""
    import torch
    from zlibstream_amd import png_expand_batch_device
    d_in = [_cuda(im["rows"].tobytes()) for im in imgs]
    d_out = [torch.empty(im["w"] * im["h"] * _px(fmt), dtype=torch.uint8, device="cuda") for im in imgs]
    torch.cuda.synchronize()
    png_expand_batch_device(engine, [t.data_ptr() for t in d_in], [im["w"] for im in imgs], [im["h"] for im in imgs], [im["depth"] for im in imgs],
                            [im["color"] for im in imgs], [t.data_ptr() for t in d_out], plte=[im["plte"] or None for im in imgs],
                            trns=[im["trns"] or None for im in imgs], format=fmt)
    return [t.cpu().numpy().tobytes() for t in d_out]


def expanded(im, fmt):
    return expand_ref(im["rows"], im["w"], im["color"], im["depth"], im["plte"], im["trns"], fmt)


# ---------------------------------------------------------------- the inverse of KX
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
@pytest.mark.parametrize("color,depth", LEGAL)
def test_pack_inverts_the_expansion(engine, color, depth, fmt):
    """raw rows -> expand_ref -> pack: the raw rows again, byte for byte, and pack_ref's bytes; the same with the device's own
    expansion in front.  (At 16 bits into RGBA8 the rows hold multiples of 257: other samples do not survive 8 bits, and
    for those the third part holds pack to pack_ref alone.)"""
    rng = np.random.default_rng(9100 + 64 * fmt + 32 * color // 2 + depth)
    imgs = [make_raw(rng, w, h, color, depth, k % 2 == 0, fmt) for k, (w, h) in enumerate(SHAPES)]
    px = [expanded(im, fmt) for im in imgs]
    got, counts = run_pack(engine, imgs, [px_bytes(p, fmt) for p in px], fmt)
    assert counts == [0] * len(imgs)
    for im, p, g in zip(imgs, px, got):
        want, miss = pack_ref(p, color, depth, im["plte"], im["trns"], fmt)
        assert miss == 0 and want.tobytes() == im["rows"].tobytes(), "the restatements are no inverses of each other"
        assert g == im["rows"].tobytes(), (im["w"], im["h"])
    dev_px = device_expand(engine, imgs, fmt)
    assert dev_px == [px_bytes(p, fmt) for p in px]
    got, _ = run_pack(engine, imgs, dev_px, fmt, unmatched=False)
    assert got == [im["rows"].tobytes() for im in imgs]
    if depth == 16 and fmt == RGBA8:
        imgs = [make_raw(rng, w, h, color, depth, k % 2 == 0, fmt, representable=False) for k, (w, h) in enumerate(SHAPES)]
        px = [expanded(im, fmt) for im in imgs]
        got, _ = run_pack(engine, imgs, [px_bytes(p, fmt) for p in px], fmt)
        for im, p, g in zip(imgs, px, got):
            assert g == pack_ref(p, color, depth, im["plte"], im["trns"], fmt)[0].tobytes(), (im["w"], im["h"])


# ---------------------------------------------------------------- pixels no file of the pair holds
def random_pixels(rng, w, h, color, depth, fmt, k):
    """random RGBA with alpha 0 on a fifth of the pixels; for a palette image a palette with duplicates and the entry
    0,0,0,0, most pixels taken from it and the others random (no entry, but by chance)"""
    top = 65535 if fmt == RGBA16 else 255
    px = rng.integers(0, top + 1, (h, w, 4)).astype(np.int64)
    px[..., 3][rng.random((h, w)) < 0.2] = 0
    px[..., 3][rng.random((h, w)) < 0.2] = top
    plte = trns = b""
    if color == 3:
        entries = (1, 2, 16, 255, 256)[k % 5]
        rgba = rng.integers(0, 256, (entries, 4), dtype=np.uint8)
        if entries > 1:
            rgba[entries // 2:, 3] = 255  # (the tRNS covers the first half)
            rgba[0] = rgba[entries - 1]   # a duplicate, alpha and all: the first is the one to be named
        if entries == 1 or entries >= 4:
            rgba[1 if entries > 1 else 0] = 0  # the entry 0, 0, 0, 0
        plte, trns = rgba[:, :3].tobytes(), rgba[:entries // 2 + (entries == 1), 3].tobytes()
        pick = _palette(plte, trns)[rng.integers(0, entries, (h, w))] * (257 if fmt == RGBA16 else 1)
        px = np.where((rng.random((h, w)) < 0.8)[..., None], pick, px)
    elif color in (0, 2) and k % 2 == 0:
        trns = bytes(rng.integers(0, 256, 2 if color == 0 else 6, dtype=np.uint8))
    return dict(w=w, h=h, color=color, depth=depth, plte=plte, trns=trns), px


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_pixels_that_no_file_of_the_pair_holds(engine, fmt):
    """truncation of the low bits, R for gray, the key under alpha 0, pixels without a palette entry: counted, index 0 written"""
    rng = np.random.default_rng(9200 + fmt)
    imgs, pxs = [], []
    for k, (c, d) in enumerate(LEGAL + [(3, 8), (3, 4), (3, 2), (3, 8), (3, 8)]):
        w, h = SHAPES[2 + k % 3]
        im, px = random_pixels(rng, w, h, c, d, fmt, k)
        imgs.append(im), pxs.append(px)
    got, counts = run_pack(engine, imgs, [px_bytes(p, fmt) for p in pxs], fmt)
    misses = 0
    for im, px, g, n in zip(imgs, pxs, got, counts):
        want, miss = pack_ref(px, im["color"], im["depth"], im["plte"], im["trns"], fmt)
        assert g == want.tobytes(), (im["color"], im["depth"], len(im["plte"]) // 3)
        assert n == miss, (im["color"], im["depth"], len(im["plte"]) // 3)
        misses += miss
    assert misses > 0 and sum(1 for n in counts if n) >= 3
    # without the counts the same bytes
    again, none = run_pack(engine, imgs, [px_bytes(p, fmt) for p in pxs], fmt, unmatched=False)
    assert again == got and none is None


# ---------------------------------------------------------------- a mixed batch
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_a_mixed_batch_at_every_alignment(engine, fmt):
    """all fifteen pairs in one call (and one more, for sixteen residues), every image another shape, the outputs carved from
    one buffer at every residue modulo 16: the same bytes as single calls and as the restatement, nothing written between"""
    import torch
    from zlibstream_amd import png_pack_batch_device
    rng = np.random.default_rng(9300 + fmt)
    imgs, pxs = [], []
    for k, (c, d) in enumerate(LEGAL + [(0, 1)]):
        im, px = random_pixels(rng, 5 + 23 * k, 1 + (7 * k) % 11, c, d, fmt, k)
        imgs.append(im), pxs.append(px)
    sizes = [_row_bytes(im["w"], im["depth"] * CHANNELS[im["color"]]) * im["h"] for im in imgs]
    offs, at = [], 0
    for k, n in enumerate(sizes):
        at = (at + GUARD + 15) // 16 * 16 + k % 16
        offs.append(at)
        at += n
    assert {o % 16 for o in offs} == set(range(16))
    buf = torch.full((at + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    d_in = [_cuda(px_bytes(p, fmt)) for p in pxs]
    torch.cuda.synchronize()
    counts = png_pack_batch_device(engine, [t.data_ptr() for t in d_in], [im["w"] for im in imgs], [im["h"] for im in imgs], [im["depth"] for im in imgs],
                                   [im["color"] for im in imgs], [buf.data_ptr() + o for o in offs], plte=[im["plte"] or None for im in imgs],
                                   trns=[im["trns"] or None for im in imgs], format=fmt, return_unmatched=True)
    b = buf.cpu().numpy().tobytes()
    at = 0
    for im, px, o, n, cnt in zip(imgs, pxs, offs, sizes, counts):
        assert b[at:o] == b"\xEE" * (o - at), "bytes between two outputs were written"
        want, miss = pack_ref(px, im["color"], im["depth"], im["plte"], im["trns"], fmt)
        assert b[o:o + n] == want.tobytes() and cnt == miss, (im["color"], im["depth"])
        single, c1 = run_pack(engine, [im], [px_bytes(px, fmt)], fmt)
        assert single[0] == want.tobytes() and c1 == [miss]
        at = o + n
    assert b[at:] == b"\xEE" * GUARD


# ---------------------------------------------------------------- the rest
def test_a_stream_of_the_caller_and_an_empty_call(engine):
    import torch
    from zlibstream_amd import png_pack_batch_device
    rng = np.random.default_rng(9400)
    s = torch.cuda.Stream()
    made = [random_pixels(rng, 257, 5, 6, 16, RGBA8, 0), random_pixels(rng, 1000, 3, 3, 2, RGBA8, 2), random_pixels(rng, 33, 31, 0, 4, RGBA8, 4)]
    got, counts = run_pack(engine, [m[0] for m in made], [px_bytes(m[1], RGBA8) for m in made], RGBA8, stream=s.cuda_stream)
    for (im, px), g, n in zip(made, got, counts):
        want, miss = pack_ref(px, im["color"], im["depth"], im["plte"], im["trns"], RGBA8)
        assert g == want.tobytes() and n == miss
    assert png_pack_batch_device(engine, [], [], [], [], [], []) is None
    assert png_pack_batch_device(engine, [], [], [], [], [], [], return_unmatched=True) == []


def test_bad_arguments_are_stream_errors_and_touch_nothing(engine):
    from zlibstream_amd import _native
    L = _native.lib()
    px = np.arange(96, dtype=np.uint8)
    d_in, d_out = _cuda(px.tobytes()), _cuda(b"\xEE" * 4096)
    VP, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    plte, trns = bytes(range(30)), bytes(range(6))
    p_plte, p_trns = ctypes.cast(ctypes.c_char_p(plte), VP).value, ctypes.cast(ctypes.c_char_p(trns), VP).value
    counts = (I64 * 2)(77, 77)

    def call(n=1, ctx=engine.handle, inp=(d_in.data_ptr(),), w=(3,), h=(4,), depth=(8,), color=(0,), pl=(p_plte,), ent=(10,), tr=(p_trns,), tl=(0,),
             fmt=RGBA8, out=(d_out.data_ptr(),), cnt=counts):
        arr = lambda t, v: None if v is None else (t * len(v))(*v)
        return L.zs_png_pack_batch_device(ctx, n, arr(VP, inp), arr(I64, w), arr(I64, h), arr(I32, depth), arr(I32, color), arr(VP, pl), arr(I32, ent),
                                          arr(VP, tr), arr(I32, tl), fmt, arr(VP, out), cnt, None)

    bad = [dict(ctx=None), dict(n=-1), dict(inp=None), dict(w=None), dict(h=None), dict(depth=None), dict(color=None), dict(out=None),
           dict(inp=(None,)), dict(out=(None,)),
           dict(color=(2,), depth=(4,)), dict(color=(3,), depth=(16,)), dict(color=(5,)), dict(color=(4,), depth=(2,)), dict(color=(6,), depth=(4,)), dict(depth=(3,)),
           dict(depth=(0,)), dict(w=(0,)), dict(w=(1 << 31,)), dict(h=(0,)), dict(h=(1 << 31,)), dict(w=(-1,)),
           dict(color=(3,), pl=None), dict(color=(3,), pl=(None,)), dict(color=(3,), ent=None), dict(color=(3,), ent=(0,)), dict(color=(3,), ent=(257,)),
           dict(color=(3,), tl=(11,)), dict(color=(3,), tl=(-1,)), dict(color=(3,), tl=(2,), tr=None), dict(color=(3,), tl=(2,), tr=(None,)),
           dict(tl=(1,)), dict(tl=(3,)), dict(tl=(6,)), dict(tl=(2,), tr=None), dict(tl=(2,), tr=(None,)),
           dict(color=(2,), w=(1,), tl=(2,)), dict(color=(2,), w=(1,), tl=(5,)), dict(color=(2,), w=(1,), tl=(6,), tr=(None,)),
           dict(fmt=2), dict(fmt=-1),
           # an input that is not aligned to its pixel
           dict(inp=(d_in.data_ptr() + 2,)), dict(inp=(d_in.data_ptr() + 1,)), dict(fmt=RGBA16, w=(1,), inp=(d_in.data_ptr() + 4,)),
           # more than 2^31 - 1 rows in one call: refused before anything is read
           dict(n=2, inp=(d_in.data_ptr(),) * 2, w=(1, 1), h=((1 << 31) - 1, 1), depth=(8, 8), color=(0, 0), pl=None, ent=None, tr=None, tl=None,
                out=(d_out.data_ptr(),) * 2)]
    for kw in bad:
        assert call(**kw) == ZS_STREAM_ERROR, kw
    assert call(n=0, inp=None, w=None, h=None, depth=None, color=None, pl=None, ent=None, tr=None, tl=None, out=None) == ZS_OK
    assert d_out.cpu().numpy().tobytes() == b"\xEE" * 4096 and list(counts) == [77, 77]
    # the same call with nothing wrong, the optional arrays absent; an output at an odd address; the counts that are ignored at
    # types 4 and 6 absurd
    rgba = px.reshape(4, 6, 4).astype(np.int64)
    assert call(w=(6,), pl=None, ent=None, tr=None, tl=None, cnt=None) == ZS_OK
    assert d_out.cpu().numpy()[:24].tobytes() == pack_ref(rgba, 0, 8, b"", b"", RGBA8)[0].tobytes()
    assert call(color=(4,), w=(6,), pl=(None,), ent=(999,), tr=(None,), tl=(77,), out=(d_out.data_ptr() + 101,)) == ZS_OK
    assert d_out.cpu().numpy()[101:149].tobytes() == pack_ref(rgba, 4, 8, b"", b"", RGBA8)[0].tobytes()
    assert list(counts) == [0, 77]


def test_the_stage_timer_shows_the_pack(engine):
    rng = np.random.default_rng(9500)
    im, px = random_pixels(rng, 257, 5, 3, 8, RGBA16, 3)
    engine.set_profiling(True)
    try:
        got, counts = run_pack(engine, [im], [px_bytes(px, RGBA16)], RGBA16)
        stages = engine.stage_ms()
    finally:
        engine.set_profiling(False)
    want, miss = pack_ref(px, 3, 8, im["plte"], im["trns"], RGBA16)
    assert got == [want.tobytes()] and counts == [miss]
    assert stages.get("png_pack", 0) > 0, stages
