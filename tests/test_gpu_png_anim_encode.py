"""Canvases to animated PNG files in one call (zs_png_encode_anim_batch_device).  The canvases are built so that the format
choice takes each of its branches; the files go back three ways -- through zs_png_decode_anim_batch, through the Python
reader of tests/png_anim_read.py and, for RGBA8, through Pillow -- and every way returns the canvases byte for byte.  Each
frame's zlib stream, cut out of its file, is what zs_png_idat_interlace_batch_device gives for that frame's cropped, packed
region alone."""
import ctypes
import io

import numpy as np
import pytest

from png_anim_read import RGBA8, RGBA16, canvases_of, diff_ref, walk
from test_gpu_png_encode_rgba import GAMA, image_for, px_bytes

pytestmark = pytest.mark.gpu

ZS_OK, ZS_STREAM_ERROR, ZS_BUF_ERROR = 0, -2, -5
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# (format, the pair the choice must land on, width, height, frames): gray opaque at 1 bit, a palette with translucent entries,
# RGB 8, gray + alpha, RGBA 8, and from RGBA16 input each 16-bit pair and one pair of 8 bits
CASES = ((RGBA8, (0, 1), 8, 8, 2), (RGBA8, (3, 4), 13, 9, 5), (RGBA8, (2, 8), 24, 16, 3), (RGBA8, (4, 8), 40, 24, 3), (RGBA8, (6, 8), 33, 17, 4),
         (RGBA16, (0, 16), 9, 8, 3), (RGBA16, (2, 16), 12, 10, 2), (RGBA16, (4, 16), 17, 11, 4), (RGBA16, (6, 16), 40, 24, 5), (RGBA16, (6, 8), 33, 17, 3))


def _px(fmt):
    return 8 if fmt == RGBA16 else 4


def _cuda(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def make_canvases(base, n_frames):
    """(h, w, 4) pixels -> (n_frames, h, w, 4): every later canvas is the one before it with pixels of `base` moved about, so
    that no canvas holds a colour the first one lacks.  Canvas 1 changes one pixel (a 1 x 1 region), canvas 2 a block five
    pixels wide, canvas 3 nothing, canvas 4 everything."""
    h, w, _ = base.shape
    cv = [base.copy()]
    for f in range(1, n_frames):
        c = cv[-1].copy()
        if f == 1:
            other = base.reshape(-1, 4)[np.nonzero((base.reshape(-1, 4) != c[h - 1, w - 1]).any(axis=1))[0][0]]
            c[h - 1, w - 1] = other
        elif f == 2:
            c[1:h - 1, 2:7] = np.roll(base, (3, 5), axis=(0, 1))[1:h - 1, 2:7]
        elif f == 4:
            c = np.roll(base, (1, 2), axis=(0, 1))
        cv.append(c)
    return np.stack(cv)


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(6100)
    out = []
    for k, (fmt, pair, w, h, nf) in enumerate(CASES):
        cv = make_canvases(image_for(pair, w, h, fmt, rng), nf)
        out.append(dict(fmt=fmt, pair=pair, w=w, h=h, cv=cv, regions=diff_ref(cv), filter=k % 6, extra=GAMA if k % 2 else b"", n_plays=k % 3,
                        delays=[(f + 1, 10 * k + f) for f in range(nf)]))
    return out


def encode_anim(engine, cs, fmt, il, caps=None, idat_chunk_bytes=0, level=6, strategy=0, stream=None):
    """-> (rc, lengths, statuses, pairs, frames, the files' bytes (None where the status is not ZS_OK))"""
    import torch
    from zlibstream_amd import png_anim_bound, png_encode_anim_batch_device
    d_in = [_cuda(px_bytes(c["cv"], fmt)) for c in cs]
    bounds = [png_anim_bound(c["w"], c["h"], len(c["cv"]), fmt, il, idat_chunk_bytes, len(c["extra"])) for c in cs]
    caps = caps or bounds
    d_out = [torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device="cuda") for cap in caps]
    torch.cuda.synchronize()
    rc, lens, st, ct, bd, frames = png_encode_anim_batch_device(engine, [t.data_ptr() for t in d_in], [len(c["cv"]) for c in cs], [c["w"] for c in cs],
                                                                [c["h"] for c in cs], [c["filter"] for c in cs], [t.data_ptr() for t in d_out], caps,
                                                                delays=[c["delays"] for c in cs], n_plays=[c["n_plays"] for c in cs], format=fmt,
                                                                interlace=[il] * len(cs), extra=[c["extra"] for c in cs], rows_per_write=3,
                                                                idat_chunk_bytes=idat_chunk_bytes, level=level, strategy=strategy, stream=stream, return_status=True)
    torch.cuda.synchronize()
    files = []
    for t, n, s, cap, b in zip(d_out, lens, st, caps, bounds):
        data = t.cpu().numpy().tobytes()
        assert data[cap:] == b"\xEE" * 64, "bytes behind an output's capacity were written"
        if s == ZS_OK:
            assert 0 < n <= cap and n <= b and data[n:cap] == b"\xEE" * (cap - n), "bytes behind a file were written, or the bound is below a length"
        else:
            assert data == b"\xEE" * len(data), "a failing animation's buffer was written"
        files.append(data[:n] if s == ZS_OK else None)
    return rc, lens, st, list(zip(ct, bd)), frames, files


@pytest.fixture(scope="module")
def encoded(engine, cases):
    """(format, interlace) -> the encode of that format's cases"""
    return {(fmt, il): encode_anim(engine, [c for c in cases if c["fmt"] == fmt], fmt, il) for fmt in (RGBA8, RGBA16) for il in (0, 1)}


def _of(cases, fmt):
    return [c for c in cases if c["fmt"] == fmt]


@pytest.mark.parametrize("il", [0, 1])
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_the_choice_takes_every_branch_and_the_regions_are_the_diff_s(engine, cases, encoded, fmt, il):
    rc, lens, st, pairs, frames, files = encoded[(fmt, il)]
    cs = _of(cases, fmt)
    assert rc == ZS_OK and st == [ZS_OK] * len(cs), engine.last_error()
    assert pairs == [c["pair"] for c in cs]
    for c, fr in zip(cs, frames):
        assert [(f["x"], f["y"], f["width"], f["height"]) for f in fr] == c["regions"]
        assert [(f["delay_num"], f["delay_den"]) for f in fr] == c["delays"] and all(f["dispose_op"] == 0 and f["blend_op"] == 0 for f in fr)
    regions = [r for c in cs for r in c["regions"][1:]]
    assert any(r[2:] == (1, 1) for r in regions) and any(1 < r[2] < 8 for r in regions), "regions of 1 x 1 and narrower than 8 pixels (absent Adam7 passes)"


@pytest.mark.parametrize("il", [0, 1])
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_the_decoder_returns_the_canvases(engine, cases, encoded, fmt, il):
    import torch
    from zlibstream_amd import png_decode_anim_batch
    files, cs = encoded[(fmt, il)][5], _of(cases, fmt)
    sizes = [c["cv"].size * (_px(fmt) // 4) for c in cs]
    d_out = [torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda") for n in sizes]
    torch.cuda.synchronize()
    st, anims = png_decode_anim_batch(engine, files, [t.data_ptr() for t in d_out], sizes, format=fmt)
    assert st == [ZS_OK] * len(cs), engine.last_error()
    for c, t, a in zip(cs, d_out, anims):
        assert (a["animated"], a["n_frames"], a["n_plays"], a["default_is_frame"], a["interlace"]) == (1, len(c["cv"]), c["n_plays"], 1, il)
        assert t.cpu().numpy().tobytes() == px_bytes(c["cv"], fmt) + b"\xEE" * 64, c["pair"]


@pytest.mark.parametrize("il", [0, 1])
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_a_python_reader_returns_the_canvases_and_finds_the_structure(cases, encoded, fmt, il):
    rc, lens, st, pairs, frames, files = encoded[(fmt, il)]
    for c, f, fr in zip(_of(cases, fmt), files, frames):
        a, got = canvases_of(f, fmt)  # (asserts every CRC, acTL in front of IDAT, the sequence numbers 0, 1, 2, ...)
        assert b"".join(got) == px_bytes(c["cv"], fmt), c["pair"]
        assert (a["width"], a["height"], a["color"], a["depth"], a["interlace"], a["n_plays"]) == (c["w"], c["h"]) + c["pair"] + (il, c["n_plays"])
        assert [(x["x"], x["y"], x["width"], x["height"]) for x in a["frames"]] == c["regions"]
        assert [(x["delay_num"], x["delay_den"]) for x in a["frames"]] == c["delays"]
        assert all((x["dispose_op"], x["blend_op"]) == (0, 0) and len(x["pieces"]) == 1 for x in a["frames"])
        assert [(len(x["stream"]), len(x["pieces"])) for x in a["frames"]] == [(x["data_bytes"], x["n_chunks"]) for x in fr]
        types = a["types"]
        assert (b"gAMA" in types) == bool(c["extra"]) and (b"PLTE" in types) == (c["pair"][0] == 3)
        if c["pair"][0] == 3:
            assert types.index(b"PLTE") < types.index(b"acTL") and (not c["extra"] or types.index(b"gAMA") < types.index(b"PLTE"))
            assert b"tRNS" in types and types.index(b"tRNS") == types.index(b"PLTE") + 1  # (the palette case has translucent entries)
        assert types.index(b"acTL") + 1 == types.index(b"fcTL") and types.index(b"fcTL") + 1 == types.index(b"IDAT")


def test_pillow_reads_the_frames(cases, encoded):
    """Every frame of the files that are not interlaced; of the interlaced ones the frame count and frame 0 only: Pillow (seen
    at 12.2) adds the interlace flag to its decoder's arguments once more per frame it loads, and so raises a TypeError on
    the second frame of any interlaced animated PNG, the hand-built ones of tests/test_gpu_png_anim.py included.  The two
    other readers cover those frames."""
    pytest.importorskip("PIL")
    from PIL import Image
    for il in (0, 1):
        for c, f in zip(_of(cases, RGBA8), encoded[(RGBA8, il)][5]):
            im = Image.open(io.BytesIO(f))
            assert im.n_frames == len(c["cv"])
            for k in range(1 if il else im.n_frames):
                im.seek(k)
                assert im.convert("RGBA").tobytes() == px_bytes(c["cv"][k], RGBA8), (c["pair"], il, k)


@pytest.mark.parametrize("level,strategy", [(0, 0), (1, 0), (6, 0), (6, 3)])
def test_every_frame_s_stream_is_the_idat_call_s_for_its_region_alone(engine, cases, level, strategy):
    """crop on the host, pack and zs_png_idat_interlace_batch_device per frame by hand: the same bytes as in the file"""
    import torch
    from zlibstream_amd import deflate_bound, png_idat_interlace_batch_device, png_idat_layout, png_pack_batch_device
    for fmt in (RGBA8, RGBA16):
        cs = _of(cases, fmt)
        for il in (0, 1):
            rc, lens, st, pairs, frames, files = encode_anim(engine, cs, fmt, il, level=level, strategy=strategy)
            assert rc == ZS_OK and st == [ZS_OK] * len(cs), engine.last_error()
            crops, ws, hs, cts, bds, plte, trns, flt, want = [], [], [], [], [], [], [], [], []
            for c, f in zip(cs, files):
                a = walk(f)
                for k, ((x, y, w, h), fr) in enumerate(zip(c["regions"], a["frames"])):
                    crops.append(_cuda(px_bytes(c["cv"][k, y:y + h, x:x + w], fmt)))
                    ws.append(w), hs.append(h), cts.append(a["color"]), bds.append(a["depth"]), flt.append(c["filter"]), want.append(fr["stream"])
                    plte.append(a["plte"] or None), trns.append(a["trns"] or None)
            bits = [d * CHANNELS[t] for t, d in zip(cts, bds)]
            d_raw = [torch.empty((w * b + 7) // 8 * h, dtype=torch.uint8, device="cuda") for w, h, b in zip(ws, hs, bits)]
            torch.cuda.synchronize()
            assert png_pack_batch_device(engine, [t.data_ptr() for t in crops], ws, hs, bds, cts, [t.data_ptr() for t in d_raw], plte=plte, trns=trns, format=fmt,
                                         return_unmatched=True) == [0] * len(crops)
            caps = [deflate_bound(png_idat_layout(w, h, b, il)[0]) for w, h, b in zip(ws, hs, bits)]
            d_z = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in caps]
            torch.cuda.synchronize()
            zl = png_idat_interlace_batch_device(engine, [t.data_ptr() for t in d_raw], ws, hs, bits, [il] * len(ws), flt, [t.data_ptr() for t in d_z], caps,
                                                 rows_per_write=3, level=level, strategy=strategy)
            torch.cuda.synchronize()
            for t, n, w in zip(d_z, zl, want):
                assert t[:n].cpu().numpy().tobytes() == w


def test_chunks_of_seven_bytes_have_consecutive_numbers_and_zero_gives_one(engine, cases, encoded):
    cs = _of(cases, RGBA8)
    rc, lens, st, pairs, frames, files = encode_anim(engine, cs, RGBA8, 1, idat_chunk_bytes=7)
    assert rc == ZS_OK and st == [ZS_OK] * len(cs), engine.last_error()
    for c, f, g, fr in zip(cs, files, encoded[(RGBA8, 1)][5], frames):
        a, b = walk(f), walk(g)  # (the walk asserts the one counter over fcTL and fdAT)
        for x, y, meta in zip(a["frames"], b["frames"], fr):
            assert x["stream"] == y["stream"] and len(y["pieces"]) == 1
            assert [len(p) for p in x["pieces"]] == [7] * (len(x["stream"]) // 7) + ([len(x["stream"]) % 7] if len(x["stream"]) % 7 else [])
            assert meta["n_chunks"] == len(x["pieces"]) > 1
        assert b"".join(canvases_of(f, RGBA8)[1]) == px_bytes(c["cv"], RGBA8)


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_one_frame_gives_the_still_encoder_s_file(engine, cases, fmt):
    import torch
    from zlibstream_amd import png_encode_rgba_batch_device
    cs = [dict(c, cv=c["cv"][:1], delays=c["delays"][:1], regions=c["regions"][:1]) for c in _of(cases, fmt)]
    for il in (0, 1):
        rc, lens, st, pairs, frames, files = encode_anim(engine, cs, fmt, il, idat_chunk_bytes=100)
        assert rc == ZS_OK and st == [ZS_OK] * len(cs), engine.last_error()
        d_in = [_cuda(px_bytes(c["cv"][0], fmt)) for c in cs]
        d_out = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in lens]
        torch.cuda.synchronize()
        still = png_encode_rgba_batch_device(engine, [t.data_ptr() for t in d_in], [c["w"] for c in cs], [c["h"] for c in cs], [c["filter"] for c in cs],
                                             [t.data_ptr() for t in d_out], lens, format=fmt, interlace=[il] * len(cs), extra=[c["extra"] for c in cs], rows_per_write=3,
                                             idat_chunk_bytes=100)
        assert still[0] == lens and list(zip(still[1], still[2])) == pairs
        for t, f in zip(d_out, files):
            assert t.cpu().numpy().tobytes() == f and b"acTL" not in f and b"fcTL" not in f


def test_a_short_capacity_fails_its_animation_only(engine, cases, encoded):
    cs = _of(cases, RGBA8)
    lens = encoded[(RGBA8, 0)][1]
    caps = list(lens)
    caps[1] -= 1
    rc, got_lens, st, pairs, frames, files = encode_anim(engine, cs, RGBA8, 0, caps=caps)  # (checks that the failing buffer keeps its guard bytes)
    assert rc == ZS_BUF_ERROR and st == [ZS_OK, ZS_BUF_ERROR] + [ZS_OK] * (len(cs) - 2) and got_lens[1] == lens[1]
    assert [f for k, f in enumerate(files) if k != 1] == [f for k, f in enumerate(encoded[(RGBA8, 0)][5]) if k != 1]


def test_a_stream_of_the_caller_and_an_empty_call(engine, cases, encoded):
    import torch
    from zlibstream_amd import png_encode_anim_batch_device
    s = torch.cuda.Stream()
    got = encode_anim(engine, _of(cases, RGBA16), RGBA16, 1, stream=s.cuda_stream)
    assert got[0] == ZS_OK and got[5] == encoded[(RGBA16, 1)][5]
    assert png_encode_anim_batch_device(engine, [], [], [], [], [], [], []) == ([], [], [], [])


def test_bad_arguments_leave_status_untouched(engine):
    from zlibstream_amd import _native
    L = _native.lib()
    d_in, d_out = _cuda(bytes(range(96)) * 2), _cuda(b"\xEE" * 4096)
    VP, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    PI32 = ctypes.POINTER(ctypes.c_int)
    p_x = ctypes.cast(ctypes.c_char_p(GAMA), VP).value
    st, lens, ct, bd = (I32 * 1)(77), (I64 * 1)(77), (I32 * 1)(77), (I32 * 1)(77)
    keep = []

    def call(n=1, ctx=engine.handle, cv=(d_in.data_ptr(),), nf=(2,), w=(3,), h=(4,), fmt=RGBA8, num=((1, 2),), den=((10, 10),), plays=(0,), flt=(0,), il=(0,),
             x=(p_x,), xl=(len(GAMA),), rpw=1, icb=0, out=(d_out.data_ptr(),), cap=(4096,), ln=lens, level=6, strategy=0):
        arr = lambda t, v: None if v is None else (t * len(v))(*v)

        def nested(v):
            if v is None:
                return None
            rows = [None if r is None else (ctypes.c_int * len(r))(*r) for r in v]
            keep.append(rows)
            return (PI32 * len(v))(*[ctypes.cast(r, PI32) if r is not None else PI32() for r in rows])

        return L.zs_png_encode_anim_batch_device(ctx, n, arr(VP, cv), arr(I32, nf), arr(I64, w), arr(I64, h), fmt, nested(num), nested(den), arr(I32, plays),
                                                 arr(I32, flt), arr(I32, il), arr(VP, x), arr(I64, xl), rpw, icb, arr(VP, out), arr(I64, cap), ln, st, None, ct, bd,
                                                 level, strategy, 0, None)

    for kw in (dict(ctx=None), dict(n=-1), dict(cv=None), dict(nf=None), dict(w=None), dict(h=None), dict(num=None), dict(den=None), dict(plays=None), dict(flt=None),
               dict(out=None), dict(cap=None), dict(ln=None), dict(xl=None), dict(cv=(None,)), dict(out=(None,)), dict(num=(None,)), dict(den=(None,)), dict(nf=(0,)),
               dict(w=(0,)), dict(w=(1 << 31,)), dict(h=(0,)), dict(h=(1 << 31,)), dict(fmt=2), dict(fmt=-1), dict(cv=(d_in.data_ptr() + 2,)),
               dict(fmt=RGBA16, w=(1,), cv=(d_in.data_ptr() + 4,)), dict(flt=(6,)), dict(flt=(-1,)), dict(il=(2,)), dict(cap=(-1,)), dict(xl=(-1,)),
               dict(xl=(len(GAMA) - 1,)), dict(x=(None,)), dict(rpw=-1), dict(icb=-1), dict(icb=1 << 31), dict(level=10), dict(level=-2), dict(strategy=5),
               dict(w=(1 << 30,), h=(1,)), dict(w=(1 << 14,), h=(1 << 15,)), dict(num=((1, 65536),)), dict(num=((-1, 2),)), dict(den=((10, 65536),)), dict(den=((10, -1),)),
               dict(plays=(-1,))):
        assert call(**kw) == ZS_STREAM_ERROR, kw
        assert (st[0], lens[0], ct[0], bd[0]) == (77, 77, 77, 77), kw
    assert call(n=0, cv=None, nf=None, w=None, h=None, num=None, den=None, plays=None, flt=None, il=None, x=None, xl=None, out=None, cap=None, ln=None) == ZS_OK
    assert d_out.cpu().numpy().tobytes() == b"\xEE" * 4096
    # nothing wrong, the optional arrays absent
    assert call(il=None, x=None, xl=None) == ZS_OK and st[0] == ZS_OK and 0 < lens[0] <= 4096
    f = d_out.cpu().numpy()[:lens[0]].tobytes()
    assert b"".join(canvases_of(f, RGBA8)[1]) == bytes(range(96)) and [(x["delay_num"], x["delay_den"]) for x in walk(f)["frames"]] == [(1, 10), (2, 10)]


def test_the_stage_timer_shows_the_diff_and_the_crop(engine, cases):
    engine.set_profiling(True)
    try:
        rc = encode_anim(engine, _of(cases, RGBA8), RGBA8, 0)[0]
        stages = engine.stage_ms()
    finally:
        engine.set_profiling(False)
    assert rc == ZS_OK and all(stages.get(k, 0) > 0 for k in ("png_survey", "png_diff", "png_crop", "png_pack", "crc32_frame")), stages
