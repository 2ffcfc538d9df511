"""Animated PNG files to composed canvases (zs_png_decode_anim_batch): the files are built here, frame by frame, for every
legal (colour type, bit depth) pair; the reference is the numpy expansion of tests/test_gpu_png_expand.py on every frame's
scanlines and the compose restatement of tests/png_anim_ref.py over them; every comparison is exact."""
import zlib

import numpy as np
import pytest

from png_anim_ref import BACKGROUND, CHANNELS, NONE, OVER, PREVIOUS, RGBA8, RGBA16, SOURCE, build_apng, chunk, compose_ref, frame_stream
from test_gpu_png_expand import LEGAL, expand_ref, make_image

pytestmark = pytest.mark.gpu

ZS_OK, ZS_STREAM_ERROR, ZS_DATA_ERROR, ZS_BUF_ERROR = 0, -2, -3, -5
GUARD = 64
W, H = 13, 9
# the frames of every file: frame 0 is the whole canvas; x, y, width, height, dispose, blend
REGIONS = ((0, 0, W, H, NONE, SOURCE), (2, 1, 9, 7, PREVIOUS, OVER), (5, 0, 8, 4, BACKGROUND, OVER), (0, 3, 6, 6, NONE, SOURCE), (12, 8, 1, 1, NONE, OVER))


def _px(fmt):
    return 8 if fmt == RGBA16 else 4


def _rows(rng, w, h, bits):
    rows = rng.integers(0, 256, (h, (w * bits + 7) // 8), dtype=np.uint8)
    if (w * bits) % 8:
        rows[:, -1] &= (0xFF00 >> ((w * bits) % 8)) & 0xFF  # (padding bits as a decoder leaves them)
    return rows


def make_anim(rng, color, depth, interlace, k, default_is_frame):
    """-> (file, description): the canvas image carries the file's PLTE / tRNS; every frame has scanlines of its own"""
    bits = depth * CHANNELS[color]
    base = make_image(rng, W, H, color, depth, with_trns=k % 2 == 0)
    if (W * bits) % 8:
        base["rows"][:, -1] &= (0xFF00 >> ((W * bits) % 8)) & 0xFF
    frames = []
    for j, (x, y, fw, fh, d, b) in enumerate(REGIONS):
        rows = base["rows"] if j == 0 else _rows(rng, fw, fh, bits)
        frames.append(dict(x=x, y=y, width=fw, height=fh, dispose_op=d, blend_op=b, rows=rows, stream=frame_stream(rows, fw, bits, interlace, k + j)))
    before = ([chunk(b"PLTE", base["plte"])] if base["plte"] else []) + ([chunk(b"tRNS", base["trns"])] if base["trns"] else [])
    default = None if default_is_frame else frame_stream(_rows(rng, W, H, bits), W, bits, interlace, k)
    f = build_apng(W, H, depth, color, interlace, frames, default_stream=default, before=before, n_plays=k, cuts=1 + k % 3,
                   between=chunk(b"tEXt", b"Comment\x00x") if k % 2 else b"")
    return f, dict(color=color, depth=depth, plte=base["plte"], trns=base["trns"], frames=frames, default_is_frame=default_is_frame)


def want_of(desc, fmt):
    frames = []
    for f in desc["frames"]:
        px = expand_ref(f["rows"], f["width"], desc["color"], desc["depth"], desc["plte"], desc["trns"], fmt)
        frames.append(dict(f, px=np.frombuffer(px, dtype="<u2" if fmt == RGBA16 else np.uint8).reshape(f["height"], f["width"], 4)))
    return b"".join(compose_ref(W, H, frames, fmt))


@pytest.fixture(scope="module")
def files():
    """every legal pair, interlaced and not, the default image a frame or not in turn -> (files, descriptions); made once"""
    rng = np.random.default_rng(8401)
    out = [make_anim(rng, c, d, il, 2 * k + il, default_is_frame=(k + il) % 3 != 0) for k, (c, d) in enumerate(LEGAL) for il in (0, 1)]
    return [f for f, _ in out], [d for _, d in out]


def decode_anim(engine, batch, fmt, caps=None, stream=None):
    """-> (statuses, anims, one bytes object per file: GUARD, the output's capacity, GUARD)"""
    import torch
    from zlibstream_amd import png_decode_anim_batch
    caps = caps or [1 << 15] * len(batch)
    d_out = [torch.full((GUARD + c + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for c in caps]
    torch.cuda.synchronize()
    st, anims = png_decode_anim_batch(engine, batch, [t.data_ptr() + GUARD for t in d_out], caps, format=fmt, stream=stream)
    torch.cuda.synchronize()
    return st, anims, [t.cpu().numpy().tobytes() for t in d_out]


def _check_output(buf, want):
    assert buf[:GUARD] == b"\xEE" * GUARD, "bytes in front of an output were written"
    assert buf[GUARD:GUARD + len(want)] == want
    assert buf[GUARD + len(want):] == b"\xEE" * (len(buf) - GUARD - len(want)), "bytes behind the canvases were written"


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_every_legal_pair_interlaced_and_not(engine, files, fmt):
    fs, descs = files
    caps = [W * H * _px(fmt) * len(REGIONS)] * len(fs)
    st, anims, got = decode_anim(engine, fs, fmt, caps=caps)
    assert st == [ZS_OK] * len(fs), engine.last_error()
    assert {a["default_is_frame"] for a in anims} == {0, 1} and {a["interlace"] for a in anims} == {0, 1}
    for d, a, g in zip(descs, anims, got):
        assert (a["animated"], a["n_frames"], a["default_is_frame"], a["color_type"], a["bit_depth"]) == (1, len(REGIONS), int(d["default_is_frame"]), d["color"], d["depth"])
        _check_output(g, want_of(d, fmt))


def test_a_stream_of_the_caller(engine, files):
    import torch
    fs, descs = files
    s = torch.cuda.Stream()
    st, _, got = decode_anim(engine, fs[:5], RGBA8, stream=s.cuda_stream)
    assert st == [ZS_OK] * 5, engine.last_error()
    for d, g in zip(descs[:5], got):
        _check_output(g, want_of(d, RGBA8))


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_a_still_file_gives_the_rgba_decode_byte_for_byte(engine, fmt):
    import torch
    from zlibstream_amd import png_decode_files_rgba_batch
    from test_gpu_png_expand import build_png
    rng = np.random.default_rng(8403)
    batch = [build_png(make_image(rng, w, h, c, d, with_trns=True), il, k=k)[0] for k, (w, h, c, d, il) in
             enumerate(((33, 31, 3, 4, 0), (21, 13, 6, 16, 1), (1, 1, 0, 1, 0), (70, 5, 2, 8, 1), (9, 40, 4, 8, 0)))]
    cap = 1 << 15
    st, anims, got = decode_anim(engine, batch, fmt, caps=[cap] * len(batch))
    assert st == [ZS_OK] * len(batch), engine.last_error()
    assert all((a["animated"], a["n_frames"], a["default_is_frame"]) == (0, 1, 1) for a in anims)
    d_out = [torch.full((GUARD + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for _ in batch]
    torch.cuda.synchronize()
    st2, infos = png_decode_files_rgba_batch(engine, batch, [t.data_ptr() + GUARD for t in d_out], [cap] * len(batch), format=fmt)
    assert st2 == [ZS_OK] * len(batch)
    for t, g, i in zip(d_out, got, infos):
        assert t.cpu().numpy().tobytes() == g and g[GUARD:GUARD + 16] != b"\xEE" * 16
        assert g[GUARD + i["width"] * i["height"] * _px(fmt):] == b"\xEE" * (len(g) - GUARD - i["width"] * i["height"] * _px(fmt))


def test_the_still_decode_of_an_animated_file_is_unchanged(engine, files):
    """zs_png_decode_files_rgba_batch steps over acTL / fcTL / fdAT as before: the default image, whether it is a frame or not"""
    import torch
    from zlibstream_amd import png_decode_files_rgba_batch
    rng = np.random.default_rng(8404)
    bits = 32
    default = _rows(rng, W, H, bits)
    other = _rows(rng, 4, 4, bits)
    fr = [dict(x=0, y=0, width=W, height=H, dispose_op=NONE, blend_op=SOURCE, stream=frame_stream(default, W, bits, 0, 1)),
          dict(x=3, y=3, width=4, height=4, dispose_op=NONE, blend_op=OVER, stream=frame_stream(other, 4, bits, 0, 2))]
    as_frame = build_apng(W, H, 8, 6, 0, fr)
    not_frame = build_apng(W, H, 8, 6, 0, fr[1:], default_stream=fr[0]["stream"])
    cap = W * H * 4
    d_out = [torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    st, infos = png_decode_files_rgba_batch(engine, [as_frame, not_frame], [t.data_ptr() for t in d_out], [cap] * 2, format=RGBA8)
    assert st == [ZS_OK] * 2, engine.last_error()
    for t in d_out:
        assert t.cpu().numpy().tobytes() == default.tobytes() + b"\xEE" * GUARD


def _flip(f, i):
    return f[:i] + bytes([f[i] ^ 0x04]) + f[i + 1:]


def test_a_file_fails_for_itself_only_and_names_the_frame(engine, files):
    fs, descs = files
    rng = np.random.default_rng(8405)
    bits = 32
    rows = [_rows(rng, W, H, bits), _rows(rng, 6, 5, bits), _rows(rng, 3, 3, bits)]
    geo = [(0, 0, W, H), (1, 2, 6, 5), (10, 6, 3, 3)]
    fr = [dict(x=x, y=y, width=w, height=h, dispose_op=NONE, blend_op=OVER, rows=r, stream=zlib.compress(b"".join(b"\x00" + bytes(l) for l in r), 0))
          for (x, y, w, h), r in zip(geo, rows)]
    good = build_apng(W, H, 8, 6, 0, fr, cuts=2)
    desc = dict(color=6, depth=8, plte=b"", trns=b"", frames=fr)
    # a bit of frame 2's second fdAT's CRC; a bit of frame 1's stream (the length of its stored block), the chunk's CRC made
    # right again; a bit of frame 1's fcTL
    last_fdat = good.rindex(b"fdAT")
    n = int.from_bytes(good[last_fdat - 4:last_fdat], "big")
    bad_crc = _flip(good, last_fdat + 4 + n + 1)
    broken = [dict(f) for f in fr]
    s = bytearray(fr[1]["stream"])
    s[3] ^= 0x04
    broken[1]["stream"] = bytes(s)
    bad_stream = build_apng(W, H, 8, 6, 0, broken, cuts=2)
    bad_fctl = _flip(good, good.index(b"fcTL", good.index(b"IDAT")) + 4 + 7)
    # a frame whose stream decodes to one row too few
    short = [dict(f) for f in fr]
    short[2]["stream"] = zlib.compress(b"".join(b"\x00" + bytes(l) for l in rows[2][:2]), 0)
    bad_len = build_apng(W, H, 8, 6, 0, short, cuts=2)
    batch = [fs[0], bad_crc, good, bad_stream, fs[3], bad_fctl, bad_len, fs[6]]
    want_st = [ZS_OK, ZS_DATA_ERROR, ZS_OK, ZS_DATA_ERROR, ZS_OK, ZS_DATA_ERROR, ZS_DATA_ERROR, ZS_OK]
    src = [descs[0], None, desc, None, descs[3], None, None, descs[6]]
    st, anims, got = decode_anim(engine, batch, RGBA8)
    assert st == want_st, engine.last_error()
    assert engine.last_error().startswith("data error: file 1: frame 2: CRC error in fdAT chunk"), engine.last_error()
    for d, g in zip(src, got):
        if d is not None:
            _check_output(g, want_of(d, RGBA8))
    # one by one, every failure names its frame
    for j, needles in ((1, ("frame 2", "CRC error in fdAT")), (3, ("frame 1:",)), (5, ("CRC error in fcTL", "frame 1")), (6, ("frame 2:",))):
        st, _, got = decode_anim(engine, [good, batch[j], fs[1]], RGBA16)
        err = engine.last_error()
        assert st == [ZS_OK, ZS_DATA_ERROR, ZS_OK] and err.startswith("data error: file 1: ") and all(x in err for x in needles), err
        _check_output(got[0], want_of(desc, RGBA16))
        _check_output(got[2], want_of(descs[1], RGBA16))


def test_a_short_capacity_fails_its_file_and_writes_nothing(engine, files):
    fs, descs = files
    need = W * H * 4 * len(REGIONS)
    st, _, got = decode_anim(engine, fs[:3], RGBA8, caps=[need, need - 1, need])
    assert st == [ZS_OK, ZS_BUF_ERROR, ZS_OK] and engine.last_error().startswith("buffer error: file 1: "), engine.last_error()
    assert got[1] == b"\xEE" * len(got[1])
    _check_output(got[0], want_of(descs[0], RGBA8))
    _check_output(got[2], want_of(descs[2], RGBA8))


def test_bad_arguments_and_an_empty_call(engine, files):
    import ctypes
    import torch
    from zlibstream_amd import _native
    L = _native.lib()
    f = files[0][0]
    d_out = torch.full((8192,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    VP, I64, I32 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_int * 1
    fp = VP(ctypes.cast(ctypes.c_char_p(f), ctypes.c_void_p).value)
    o, n, cap = VP(d_out.data_ptr()), I64(len(f)), I64(8192)
    for a in ((-1, fp, n, RGBA8, o, cap), (1, None, n, RGBA8, o, cap), (1, fp, None, RGBA8, o, cap), (1, fp, n, RGBA8, None, cap), (1, fp, n, RGBA8, o, None),
              (1, VP(None), n, RGBA8, o, cap), (1, fp, I64(-1), RGBA8, o, cap), (1, fp, n, RGBA8, VP(None), cap), (1, fp, n, RGBA8, o, I64(-1)),
              (1, fp, n, 2, o, cap), (1, fp, n, -1, o, cap), (1, fp, n, RGBA8, VP(d_out.data_ptr() + 2), cap), (1, fp, n, RGBA16, VP(d_out.data_ptr() + 4), cap)):
        st = I32(77)
        assert L.zs_png_decode_anim_batch(engine.handle, a[0], a[1], a[2], a[3], a[4], a[5], None, st, None) == ZS_STREAM_ERROR and st[0] == 77, a
    assert L.zs_png_decode_anim_batch(None, 1, fp, n, RGBA8, o, cap, None, None, None) == ZS_STREAM_ERROR
    assert L.zs_png_decode_anim_batch(engine.handle, 0, None, None, RGBA8, None, None, None, None, None) == ZS_OK
    assert d_out.cpu().numpy().tobytes() == b"\xEE" * 8192


def test_the_stage_timer_shows_the_compose_launch(engine, files):
    engine.set_profiling(True)
    try:
        st, _, _ = decode_anim(engine, files[0][:4], RGBA8)
        ms = engine.stage_ms()
    finally:
        engine.set_profiling(False)
    assert st == [ZS_OK] * 4
    assert ms.get("png_compose", 0) > 0 and ms.get("png_expand", 0) > 0 and ms.get("crc32_frame", 0) > 0, ms
