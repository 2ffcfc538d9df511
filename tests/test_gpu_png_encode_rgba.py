"""RGBA pixels to PNG files in one call (zs_png_encode_rgba_batch_device): survey, choice, PLTE / tRNS, pack, then the
interlace-encode body.  Fifteen images built so that the choice lands on each legal (colour type, bit depth) pair; the files go
back through the existing decoder and expander -- neither is code under test -- and equal the source pixels exactly, and each
file equals, byte for byte, what png_encode_interlace_batch_device writes from png_pack_batch_device's output."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZS_OK, ZS_STREAM_ERROR, ZS_BUF_ERROR = 0, -2, -5
RGBA8, RGBA16 = 0, 1
LEGAL = [(c, d) for c, ds in ((0, (1, 2, 4, 8, 16)), (2, (8, 16)), (3, (1, 2, 4, 8)), (4, (8, 16)), (6, (8, 16))) for d in ds]
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
GAMA = struct.pack(">I", 4) + b"gAMA" + struct.pack(">I", 45455) + struct.pack(">I", zlib.crc32(b"gAMA" + struct.pack(">I", 45455)))


def chunk(ctype, data):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data))


def _px(fmt):
    return 8 if fmt == RGBA16 else 4


def image_for(pair, w, h, fmt, rng):
    """(h, w, 4) int64 pixels of format fmt on which the rule chooses `pair`, or None where no image of that format can"""
    color, depth = pair
    if depth == 16 and fmt == RGBA8:
        return None
    n = w * h
    i = np.arange(n)
    top = 65535 if fmt == RGBA16 else 255
    px = np.zeros((n, 4), dtype=np.int64)
    if depth == 16:  # samples that are no multiples of 257
        px[:] = rng.integers(0, 65536, (n, 4))
        px[0] = (0x1234, 0x0102, 0xFFFE, 0x00FF)
        if color in (0, 4):
            px[:, 1] = px[:, 2] = px[:, 0]
        if color in (0, 2):
            px[:, 3] = top
        return px.reshape(h, w, 4)
    m = 257 if fmt == RGBA16 else 1
    px[:, 3] = 255
    if color == 0:
        levels = {1: 2, 2: 4, 4: 16, 8: 200}[depth]  # (all of them present: a palette of them is no narrower)
        v = rng.permutation(np.concatenate([np.arange(levels), rng.integers(0, levels, n - levels)]))
        px[:, 0] = px[:, 1] = px[:, 2] = v * (255 // (levels - 1)) if depth < 8 else v + 20
    elif color == 2:
        px[:, 0], px[:, 1], px[:, 2] = i & 255, i >> 8, 7  # more than 256 colours
    elif color == 4:
        px[:, 0] = px[:, 1] = px[:, 2] = i & 255
        px[:, 3] = 254 - (i >> 8)  # more than 256 pairs
    elif color == 6:
        px[:, 0], px[:, 1], px[:, 2], px[:, 3] = i & 255, 3, i >> 8, 255 - (i & 1)
    else:
        if depth == 1:
            pal = np.array([(200, 0, 0, 255), (0, 0, 200, 255)])  # two colours that are not gray
        elif depth == 2:
            pal = np.array([(10, 10, 10, 255), (20, 20, 20, 255), (30, 30, 30, 255)])  # three grays that are no multiples of 85, all opaque
        elif depth == 4:
            pal = rng.integers(0, 256, (10, 4))
            pal[:, 0] = np.arange(10)  # (different)
            pal[:, 3] = 255
            pal[[2, 5, 7], 3] = (0, 254, 100)  # three translucent colours
        else:
            pal = rng.integers(0, 256, (100, 4))
            pal[:, 0] = np.arange(100)
        px[:] = pal[rng.permutation(np.concatenate([np.arange(len(pal)), rng.integers(0, len(pal), n - len(pal))]))]
    return px.reshape(h, w, 4) * m


def px_bytes(px, fmt):
    return px.astype("<u2" if fmt == RGBA16 else np.uint8).tobytes()


def _cuda(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def bound(w, h, fmt, il, extra_len, idat_chunk_bytes=0):
    from zlibstream_amd import deflate_bound, png_file_bound, png_idat_layout
    return png_file_bound(deflate_bound(png_idat_layout(w, h, 8 * _px(fmt), il)[0]), idat_chunk_bytes, extra_len + 1048)


@pytest.fixture(scope="module")
def cases():
    """fmt -> a list of dict(pair, px, w, h, il, extra, filter): every pair the format can reach, interlaced and not"""
    out = {}
    for fmt in (RGBA8, RGBA16):
        rng = np.random.default_rng(9700 + fmt)
        lst = []
        for k, pair in enumerate(LEGAL):
            for il, (w, h) in ((0, (33, 31)), (1, (21, 13))):
                px = image_for(pair, w, h, fmt, rng)
                if px is not None:
                    lst.append(dict(pair=pair, px=px, w=w, h=h, il=il, extra=GAMA if (k + il) % 2 else b"", filter=(k + il) % 6))
        out[fmt] = lst
    assert {c["pair"] for c in out[RGBA16]} == set(LEGAL) and {c["pair"] for c in out[RGBA8]} == {p for p in LEGAL if p[1] != 16}
    return out


def encode_rgba(engine, cs, fmt, caps=None, idat_chunk_bytes=0, stream=None):
    """-> (rc, lengths, statuses, color types, bit depths, the files' bytes (None where the status is not ZS_OK))"""
    import torch
    from zlibstream_amd import png_encode_rgba_batch_device
    d_in = [_cuda(px_bytes(c["px"], fmt)) for c in cs]
    caps = caps or [bound(c["w"], c["h"], fmt, c["il"], len(c["extra"]), idat_chunk_bytes) for c in cs]
    d_out = [torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device="cuda") for cap in caps]
    torch.cuda.synchronize()
    rc, lens, st, ct, bd = png_encode_rgba_batch_device(engine, [t.data_ptr() for t in d_in], [c["w"] for c in cs], [c["h"] for c in cs],
                                                        [c["filter"] for c in cs], [t.data_ptr() for t in d_out], caps, format=fmt,
                                                        interlace=[c["il"] for c in cs], extra=[c["extra"] for c in cs], rows_per_write=3,
                                                        idat_chunk_bytes=idat_chunk_bytes, stream=stream, return_status=True)
    torch.cuda.synchronize()
    files = []
    for t, n, s, cap in zip(d_out, lens, st, caps):
        b = t.cpu().numpy().tobytes()
        assert b[cap:] == b"\xEE" * 64, "bytes behind an output's capacity were written"
        if s == ZS_OK:
            assert 0 < n <= cap and b[n:cap] == b"\xEE" * (cap - n), "bytes behind a file were written"
        else:
            assert b == b"\xEE" * len(b)
        files.append(b[:n] if s == ZS_OK else None)
    return rc, lens, st, ct, bd, files


def chunks_of(f):
    out, at = [], 8
    while at < len(f):
        n = int.from_bytes(f[at:at + 4], "big")
        out.append((f[at + 4:at + 8], f[at + 8:at + 8 + n]))
        at += 12 + n
    return out


@pytest.fixture(scope="module")
def encoded(engine, cases):
    return {fmt: encode_rgba(engine, cases[fmt], fmt) for fmt in (RGBA8, RGBA16)}


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_the_choice_lands_on_every_pair_and_the_files_say_so(engine, cases, encoded, fmt):
    from zlibstream_amd import png_file_info
    rc, lens, st, ct, bd, files = encoded[fmt]
    assert rc == ZS_OK and st == [ZS_OK] * len(files), engine.last_error()
    for c, f, t, d in zip(cases[fmt], files, ct, bd):
        info = png_file_info(f)
        assert (t, d) == c["pair"], (c["pair"], c["il"])
        assert (info["color_type"], info["bit_depth"], info["interlace"], info["width"], info["height"]) == (t, d, c["il"], c["w"], c["h"])


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_the_files_decode_to_the_source_pixels(engine, cases, encoded, fmt):
    import torch
    from zlibstream_amd import png_decode_files_rgba_batch
    files = encoded[fmt][5]
    sizes = [c["w"] * c["h"] * _px(fmt) for c in cases[fmt]]
    d_out = [torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda") for n in sizes]
    torch.cuda.synchronize()
    st, infos = png_decode_files_rgba_batch(engine, files, [t.data_ptr() for t in d_out], sizes, format=fmt)
    assert st == [ZS_OK] * len(files), engine.last_error()
    for c, t, n in zip(cases[fmt], d_out, sizes):
        assert t.cpu().numpy().tobytes() == px_bytes(c["px"], fmt) + b"\xEE" * 64, (c["pair"], c["il"])


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_the_files_are_the_interlace_encoders_from_the_packed_scanlines(engine, cases, encoded, fmt):
    """survey, choice, PLTE / tRNS, pack and png_encode_interlace_batch_device done by hand give the same bytes"""
    import torch
    from zlibstream_amd import png_choose_format, png_encode_interlace_batch_device, png_pack_batch_device, png_survey_batch_device
    cs, files = cases[fmt], encoded[fmt][5]
    d_in = [_cuda(px_bytes(c["px"], fmt)) for c in cs]
    ws, hs = [c["w"] for c in cs], [c["h"] for c in cs]
    surveys = png_survey_batch_device(engine, [t.data_ptr() for t in d_in], ws, hs, format=fmt)
    pairs = [png_choose_format(s) for s in surveys]
    assert pairs == [c["pair"] for c in cs]
    plte, trns, extra = [], [], []
    for c, s, (ct, bd) in zip(cs, surveys, pairs):
        p = t = None
        x = c["extra"]
        if ct == 3:
            p = b"".join(bytes(col[:3]) for col in s["colors"])
            alphas = [col[3] for col in s["colors"]]
            while alphas and alphas[-1] == 255:
                alphas.pop()
            t = bytes(alphas) or None
            x = x + chunk(b"PLTE", p) + (chunk(b"tRNS", t) if t else b"")
        plte.append(p), trns.append(t), extra.append(x)
    sizes = [(w * bd * CHANNELS[ct] + 7) // 8 * h for w, h, (ct, bd) in zip(ws, hs, pairs)]
    d_raw = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in sizes]
    torch.cuda.synchronize()
    assert png_pack_batch_device(engine, [t.data_ptr() for t in d_in], ws, hs, [p[1] for p in pairs], [p[0] for p in pairs], [t.data_ptr() for t in d_raw],
                                 plte=plte, trns=trns, format=fmt, return_unmatched=True) == [0] * len(cs)
    caps = [len(f) for f in files]
    d_out = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in caps]
    torch.cuda.synchronize()
    lens = png_encode_interlace_batch_device(engine, [t.data_ptr() for t in d_raw], ws, hs, [p[1] for p in pairs], [p[0] for p in pairs],
                                             [c["filter"] for c in cs], [t.data_ptr() for t in d_out], caps, interlace=[c["il"] for c in cs], extra=extra,
                                             rows_per_write=3)
    assert lens == caps
    for c, t, f in zip(cs, d_out, files):
        assert t.cpu().numpy().tobytes() == f, (c["pair"], c["il"])


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_plte_and_trns_are_the_surveys_colours(engine, cases, encoded, fmt):
    """a palette whose colours are all opaque has no tRNS chunk; the one with three translucent colours has a tRNS of 3 bytes;
    the caller's chunk stands in front of PLTE"""
    files = encoded[fmt][5]
    seen = set()
    for c, f in zip(cases[fmt], files):
        ch = chunks_of(f)
        types = [t for t, _ in ch]
        assert types[0] == b"IHDR" and types[-1] == b"IEND" and types.count(b"IDAT") == 1
        assert (b"gAMA" in types) == bool(c["extra"])
        if c["pair"][0] != 3:
            assert b"PLTE" not in types and b"tRNS" not in types
            continue
        colors = np.unique((c["px"] // (257 if fmt == RGBA16 else 1)).reshape(-1, 4), axis=0)
        colors = colors[np.lexsort((colors[:, 2], colors[:, 1], colors[:, 0], colors[:, 3]))]
        assert dict(ch)[b"PLTE"] == colors[:, :3].astype(np.uint8).tobytes()
        n_trns = int(np.count_nonzero(colors[:, 3] != 255))  # (ascending by alpha: the translucent ones come first)
        if n_trns == 0:
            assert b"tRNS" not in types
        else:
            assert dict(ch)[b"tRNS"] == colors[:n_trns, 3].astype(np.uint8).tobytes()
            assert types.index(b"PLTE") + 1 == types.index(b"tRNS")
        if c["extra"]:
            assert types.index(b"gAMA") < types.index(b"PLTE")
        assert types.index(b"PLTE") < types.index(b"IDAT")
        seen.add((c["pair"][1], n_trns))
    assert {(1, 0), (2, 0), (4, 3)} <= seen and any(d == 8 and n > 3 for d, n in seen)


def test_idat_chunks_a_stream_of_the_caller_and_an_empty_call(engine, cases):
    import torch
    from zlibstream_amd import png_encode_rgba_batch_device
    cs = cases[RGBA16][::5]
    s = torch.cuda.Stream()
    rc, lens, st, ct, bd, files = encode_rgba(engine, cs, RGBA16, idat_chunk_bytes=100, stream=s.cuda_stream)
    assert rc == ZS_OK and st == [ZS_OK] * len(cs) and list(zip(ct, bd)) == [c["pair"] for c in cs]
    whole = encode_rgba(engine, cs, RGBA16)[5]
    for f, g in zip(files, whole):
        a, b = chunks_of(f), chunks_of(g)
        assert all(len(d) <= 100 for t, d in a if t == b"IDAT")
        assert b"".join(d for t, d in a if t == b"IDAT") == b"".join(d for t, d in b if t == b"IDAT")
        assert [x for x in a if x[0] != b"IDAT"] == [x for x in b if x[0] != b"IDAT"]
    assert png_encode_rgba_batch_device(engine, [], [], [], [], [], []) == ([], [], [])


def test_a_capacity_one_byte_short_fails_that_image_alone(engine, cases, encoded):
    cs = cases[RGBA8][:6]
    lens = encoded[RGBA8][1][:6]
    caps = list(lens)
    caps[2] -= 1
    rc, got_lens, st, ct, bd, files = encode_rgba(engine, cs, RGBA8, caps=caps)
    assert rc == ZS_BUF_ERROR and st == [ZS_OK, ZS_OK, ZS_BUF_ERROR, ZS_OK, ZS_OK, ZS_OK]
    assert [f for k, f in enumerate(files) if k != 2] == [f for k, f in enumerate(encoded[RGBA8][5][:6]) if k != 2]
    assert list(zip(ct, bd)) == [c["pair"] for c in cs]


def test_bad_arguments_leave_status_untouched(engine):
    from zlibstream_amd import _native
    L = _native.lib()
    d_in, d_out = _cuda(bytes(range(96))), _cuda(b"\xEE" * 4096)
    VP, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    p_x = ctypes.cast(ctypes.c_char_p(GAMA), VP).value
    st, lens, ct, bd = (I32 * 1)(77), (I64 * 1)(77), (I32 * 1)(77), (I32 * 1)(77)

    def call(n=1, ctx=engine.handle, px=(d_in.data_ptr(),), w=(3,), h=(4,), fmt=RGBA8, flt=(0,), il=(0,), x=(p_x,), xl=(len(GAMA),), rpw=1, icb=0,
             out=(d_out.data_ptr(),), cap=(4096,), ln=lens, level=6, strategy=0):
        arr = lambda t, v: None if v is None else (t * len(v))(*v)
        return L.zs_png_encode_rgba_batch_device(ctx, n, arr(VP, px), arr(I64, w), arr(I64, h), fmt, arr(I32, flt), arr(I32, il), arr(VP, x), arr(I64, xl),
                                                 rpw, icb, arr(VP, out), arr(I64, cap), ln, st, ct, bd, level, strategy, 0, None)

    for kw in (dict(ctx=None), dict(n=-1), dict(px=None), dict(w=None), dict(h=None), dict(flt=None), dict(out=None), dict(cap=None), dict(ln=None), dict(xl=None),
               dict(px=(None,)), dict(out=(None,)), dict(w=(0,)), dict(w=(1 << 31,)), dict(h=(0,)), dict(h=(1 << 31,)), dict(fmt=2), dict(fmt=-1),
               dict(px=(d_in.data_ptr() + 2,)), dict(fmt=RGBA16, w=(1,), px=(d_in.data_ptr() + 4,)), dict(flt=(6,)), dict(flt=(-1,)), dict(il=(2,)), dict(cap=(-1,)),
               dict(xl=(-1,)), dict(xl=(len(GAMA) - 1,)), dict(x=(None,)), dict(rpw=-1), dict(icb=-1), dict(icb=1 << 31), dict(level=10), dict(level=-2),
               dict(strategy=5), dict(w=(1 << 30,), h=(1 << 30,))):
        assert call(**kw) == ZS_STREAM_ERROR, kw
        assert (st[0], lens[0], ct[0], bd[0]) == (77, 77, 77, 77), kw
    assert call(n=0, px=None, w=None, h=None, flt=None, il=None, x=None, xl=None, out=None, cap=None, ln=None) == ZS_OK
    assert d_out.cpu().numpy().tobytes() == b"\xEE" * 4096
    # nothing wrong, the optional arrays absent
    assert call(il=None, x=None, xl=None) == ZS_OK and st[0] == ZS_OK and 0 < lens[0] <= 4096 and (ct[0], bd[0]) == (3, 4)
    assert d_out.cpu().numpy()[:8].tobytes() == b"\x89PNG\r\n\x1a\n"


def test_the_stage_timer_shows_the_front_end(engine, cases):
    engine.set_profiling(True)
    try:
        rc = encode_rgba(engine, cases[RGBA8][:4], RGBA8)[0]
        stages = engine.stage_ms()
    finally:
        engine.set_profiling(False)
    assert rc == ZS_OK and stages.get("png_survey", 0) > 0 and stages.get("png_pack", 0) > 0 and stages.get("crc32_frame", 0) > 0, stages


def test_pillow_reads_the_files(engine, cases, encoded):
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    for c, f in zip(cases[RGBA8], encoded[RGBA8][5]):
        assert Image.open(io.BytesIO(f)).convert("RGBA").tobytes() == px_bytes(c["px"], RGBA8), (c["pair"], c["il"])
