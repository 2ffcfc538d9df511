"""Animated PNG, the parts that need no GPU: zs_png_anim_info -- pure host code -- on hand-built files through ctypes, and the
numpy restatement of the compose rules (tests/png_anim_ref.py), which the GPU tests compare the device with, against
Pillow's own frame-by-frame decode of files Pillow wrote."""
import ctypes
import io
import struct
import zlib

import numpy as np
import pytest

from png_anim_ref import (BACKGROUND, IEND, NONE, OVER, PREVIOUS, RGBA8, SIG, SOURCE, actl, chunk, compose_ref, fctl, fctl_data, fdat, flipped,
                          ihdr)

ZS_OK, ZS_STREAM_ERROR, ZS_DATA_ERROR, ZS_BUF_ERROR = 0, -2, -3, -5
W, H = 4, 3


def stream(w=W, h=H):
    return zlib.compress(bytes(h * (w * 4 + 1)))


IDAT = chunk(b"IDAT", stream())
TEXT = chunk(b"tEXt", b"Comment\x00between")


def png(*parts):
    return SIG + ihdr(W, H) + b"".join(parts) + IEND


def anim_info(f, cap=16):
    """-> (rc, anim, frames) straight from the C entry point"""
    from zlibstream_amd import _native
    anim = _native.PngAnim()
    frames = (_native.PngFrame * max(cap, 1))()
    rc = _native.lib().zs_png_anim_info(f, len(f), ctypes.byref(anim), frames if cap else None, cap)
    return rc, anim, frames


def test_a_still_file_is_one_frame():
    from zlibstream_amd import png_anim_info, png_file_info
    # (its fcTL and fdAT chunks mean nothing without an acTL: stepped over, whatever they hold)
    f = png(chunk(b"fcTL", b"junk"), chunk(b"IDAT", stream()[:5]), chunk(b"IDAT", stream()[5:]), chunk(b"fdAT", b""), fctl(9, 99, 99))
    rc, anim, frames = anim_info(f)
    assert rc == ZS_OK
    assert (anim.animated, anim.n_frames, anim.n_plays, anim.default_is_frame) == (0, 1, 0, 1)
    fr = frames[0]
    assert (fr.x, fr.y, fr.width, fr.height, fr.dispose_op, fr.blend_op) == (0, 0, W, H, NONE, SOURCE)
    assert (fr.data_bytes, fr.n_chunks) == (len(stream()), 2)
    a, fs = png_anim_info(f)
    assert {k: a[k] for k in png_file_info(f)} == png_file_info(f) and a["n_frames"] == 1 and len(fs) == 1 and fs[0]["width"] == W


def test_the_default_image_as_frame_0():
    from zlibstream_amd import png_anim_info
    s1 = zlib.compress(bytes(2 * (2 * 4 + 1)))
    f = png(actl(2, 7), fctl(0, W, H, delay_num=3, delay_den=0, dispose=BACKGROUND, blend=OVER), IDAT,
            fctl(1, 2, 2, x=2, y=1, delay_num=65535, delay_den=100, dispose=PREVIOUS), fdat(2, s1))
    a, fs = png_anim_info(f)
    assert (a["animated"], a["n_frames"], a["n_plays"], a["default_is_frame"], a["width"], a["height"], a["color_type"]) == (1, 2, 7, 1, W, H, 6)
    assert fs[0] == dict(x=0, y=0, width=W, height=H, delay_num=3, delay_den=0, dispose_op=BACKGROUND, blend_op=OVER, data_bytes=len(stream()), n_chunks=1)
    assert fs[1] == dict(x=2, y=1, width=2, height=2, delay_num=65535, delay_den=100, dispose_op=PREVIOUS, blend_op=SOURCE, data_bytes=len(s1), n_chunks=1)
    # the acTL may stand behind the default image's fcTL: the specification orders both against IDAT only
    assert png_anim_info(png(fctl(0, W, H), actl(1), IDAT))[0]["default_is_frame"] == 1


def test_the_default_image_not_a_frame():
    from zlibstream_amd import png_anim_info
    f = png(actl(2), IDAT, fctl(0, W, H), fdat(1, stream()), fctl(2, 1, 1, x=3, y=2), fdat(3, zlib.compress(bytes(5))))
    a, fs = png_anim_info(f)
    assert (a["animated"], a["n_frames"], a["default_is_frame"], a["idat_bytes"]) == (1, 2, 0, len(stream()))
    assert [(x["x"], x["y"], x["width"], x["height"], x["data_bytes"]) for x in fs] == [(0, 0, W, H, len(stream())), (3, 2, 1, 1, len(zlib.compress(bytes(5))))]


def test_several_fdats_a_frame_with_a_text_chunk_between_them():
    from zlibstream_amd import png_anim_info
    s = stream()
    f = png(actl(2), fctl(0, W, H), IDAT, TEXT, fctl(1, W, H), fdat(2, s[:3]), TEXT, fdat(3, s[3:4]), chunk(b"zzZz", b"x" * 9), fdat(4, b""), fdat(5, s[4:]), TEXT)
    a, fs = png_anim_info(f)
    assert a["n_frames"] == 2 and (fs[1]["data_bytes"], fs[1]["n_chunks"]) == (len(s), 4) and (fs[0]["data_bytes"], fs[0]["n_chunks"]) == (len(s), 1)


S = stream()
S1 = zlib.compress(bytes(5))
REJECTED = {
    "acTL: a second one": png(actl(1), actl(1), fctl(0, W, H), IDAT),
    "acTL: 7 bytes": png(chunk(b"acTL", bytes(7)), fctl(0, W, H), IDAT),
    "acTL: 9 bytes": png(chunk(b"acTL", struct.pack(">II", 1, 0) + b"\x00"), fctl(0, W, H), IDAT),
    "acTL: behind the first IDAT": png(IDAT, actl(1), fctl(0, W, H), fdat(1, S)),
    "acTL: num_frames 0": png(actl(0), IDAT),
    "acTL: num_frames 2^31": png(actl(1 << 31), fctl(0, W, H), IDAT),
    "acTL: a wrong CRC": png(flipped(b"acTL", struct.pack(">II", 1, 0)), fctl(0, W, H), IDAT),
    "fcTL: 25 bytes": png(actl(1), chunk(b"fcTL", fctl_data(0, W, H)[:25]), IDAT),
    "fcTL: 27 bytes": png(actl(1), chunk(b"fcTL", fctl_data(0, W, H) + b"\x00"), IDAT),
    "fcTL: the first sequence number is 1": png(actl(1), fctl(1, W, H), IDAT),
    "fcTL: a sequence number twice": png(actl(2), fctl(0, W, H), IDAT, fctl(0, W, H), fdat(1, S)),
    "fcTL: a sequence number left out": png(actl(2), fctl(0, W, H), IDAT, fctl(2, W, H), fdat(3, S)),
    "fcTL: a sequence number that ignores the fdATs": png(actl(3), fctl(0, W, H), IDAT, fctl(1, W, H), fdat(2, S), fctl(2, W, H), fdat(3, S)),
    "fcTL: two in front of IDAT": png(actl(2), fctl(0, W, H), fctl(1, W, H), IDAT),
    "fcTL: in front of IDAT and narrower than the canvas": png(actl(1), fctl(0, W - 1, H), IDAT),
    "fcTL: in front of IDAT and lower than the canvas": png(actl(1), fctl(0, W, H - 1), IDAT),
    "fcTL: in front of IDAT at x = 1": png(actl(1), fctl(0, W - 1, H, x=1), IDAT),
    "fcTL: in front of IDAT at y = 1": png(actl(1), fctl(0, W, H - 1, y=1), IDAT),
    "fcTL: two in a row": png(actl(3), fctl(0, W, H), IDAT, fctl(1, W, H), fctl(2, W, H), fdat(3, S)),
    "fcTL: the last one has no data": png(actl(2), fctl(0, W, H), IDAT, fctl(1, W, H)),
    "fcTL: the only one behind IDAT has no data": png(actl(1), IDAT, fctl(0, W, H), TEXT),
    "fcTL: width 0": png(actl(2), fctl(0, W, H), IDAT, fctl(1, 0, 1), fdat(2, S1)),
    "fcTL: height 0": png(actl(2), fctl(0, W, H), IDAT, fctl(1, 1, 0), fdat(2, S1)),
    "fcTL: x + width beyond the canvas": png(actl(2), fctl(0, W, H), IDAT, fctl(1, 2, 1, x=W - 1), fdat(2, S1)),
    "fcTL: y + height beyond the canvas": png(actl(2), fctl(0, W, H), IDAT, fctl(1, 1, 2, y=H - 1), fdat(2, S1)),
    "fcTL: x of 2^32 - 1": png(actl(2), fctl(0, W, H), IDAT, fctl(1, 1, 1, x=0xFFFFFFFF), fdat(2, S1)),
    "fcTL: dispose 3": png(actl(1), fctl(0, W, H, dispose=3), IDAT),
    "fcTL: blend 2": png(actl(1), fctl(0, W, H, blend=2), IDAT),
    "fcTL: a wrong CRC": png(actl(1), flipped(b"fcTL", fctl_data(0, W, H)), IDAT),
    "fcTL: a wrong CRC behind IDAT": png(actl(2), fctl(0, W, H), IDAT, flipped(b"fcTL", fctl_data(1, W, H)), fdat(2, S)),
    "fdAT: 3 bytes": png(actl(2), fctl(0, W, H), IDAT, fctl(1, W, H), chunk(b"fdAT", b"\x00\x00\x00")),
    "fdAT: empty": png(actl(2), fctl(0, W, H), IDAT, fctl(1, W, H), chunk(b"fdAT", b"")),
    "fdAT: the wrong sequence number": png(actl(2), fctl(0, W, H), IDAT, fctl(1, W, H), fdat(3, S)),
    "fdAT: the second one repeats the first one's number": png(actl(2), fctl(0, W, H), IDAT, fctl(1, W, H), fdat(2, S[:4]), fdat(2, S[4:])),
    "fdAT: in front of IDAT": png(actl(1), fctl(0, W, H), fdat(1, S), IDAT),
    "fdAT: no fcTL since IDAT": png(actl(1), fctl(0, W, H), IDAT, fdat(1, S)),
    "fdAT: no fcTL at all": png(actl(1), IDAT, fdat(0, S)),
    "frames: one fcTL fewer than num_frames": png(actl(3), fctl(0, W, H), IDAT, fctl(1, W, H), fdat(2, S)),
    "frames: one fcTL more than num_frames": png(actl(1), fctl(0, W, H), IDAT, fctl(1, W, H), fdat(2, S)),
    "frames: no fcTL": png(actl(1), IDAT),
    "what zs_png_file_info rejects: a wrong IDAT CRC": png(actl(1), fctl(0, W, H), flipped(b"IDAT", S)),
    "what zs_png_file_info rejects: no IEND": png(actl(1), fctl(0, W, H), IDAT)[:-12],
    "what zs_png_file_colors rejects: a second tRNS": SIG + ihdr(W, H, 8, 0) + chunk(b"tRNS", bytes(2)) * 2 + actl(1) + fctl(0, W, H) + IDAT + IEND,
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_every_rejection_has_its_file(case):
    from zlibstream_amd import ZlibStreamException, png_anim_info
    rc, _, _ = anim_info(REJECTED[case])
    assert rc == ZS_DATA_ERROR
    with pytest.raises(ZlibStreamException):
        png_anim_info(REJECTED[case])


def test_the_rejections_differ_from_a_good_file_in_what_they_name_only():
    """every family's good neighbour is taken: the files above fail for the reason in their names"""
    good = [png(actl(1), fctl(0, W, H), IDAT), png(actl(2), fctl(0, W, H), IDAT, fctl(1, W, H), fdat(2, S)),
            png(actl(2), fctl(0, W, H), IDAT, fctl(1, 1, 1, x=W - 1, y=H - 1, dispose=2, blend=1), fdat(2, S1)),
            png(actl(3), fctl(0, W, H), IDAT, fctl(1, W, H), fdat(2, S), fctl(3, W, H), fdat(4, S)), png(actl(1), IDAT, fctl(0, W, H), fdat(1, S)),
            png(actl(2), fctl(0, W, H), IDAT, fctl(1, W, H), fdat(2, S[:4]), fdat(3, S[4:])),
            # an fdAT's own CRC is not read on the host: the device checks it
            png(actl(2), fctl(0, W, H), IDAT, fctl(1, W, H), flipped(b"fdAT", struct.pack(">I", 2) + S))]
    for f in good:
        assert anim_info(f)[0] == ZS_OK


def test_frames_cap_too_small_and_null_arguments():
    from zlibstream_amd import _native
    L = _native.lib()
    f = png(actl(3), fctl(0, W, H), IDAT, fctl(1, 2, 1), fdat(2, S1), fctl(3, 1, 2, x=1), fdat(4, S1))
    rc, anim, frames = anim_info(f, cap=2)
    assert rc == ZS_BUF_ERROR and (anim.animated, anim.n_frames, anim.png.width) == (1, 3, W)
    assert (frames[0].width, frames[1].width, frames[1].height) == (W, 2, 1)
    rc, anim, _ = anim_info(f, cap=0)
    assert rc == ZS_BUF_ERROR and anim.n_frames == 3
    assert anim_info(f, cap=3)[0] == ZS_OK
    anim, frames = _native.PngAnim(), (_native.PngFrame * 4)()
    assert L.zs_png_anim_info(None, len(f), ctypes.byref(anim), frames, 4) == ZS_STREAM_ERROR
    assert L.zs_png_anim_info(f, len(f), None, frames, 4) == ZS_STREAM_ERROR
    assert L.zs_png_anim_info(f, -1, ctypes.byref(anim), frames, 4) == ZS_STREAM_ERROR
    assert L.zs_png_anim_info(f, len(f), ctypes.byref(anim), None, 4) == ZS_STREAM_ERROR
    assert L.zs_png_anim_info(f, len(f), ctypes.byref(anim), frames, -1) == ZS_STREAM_ERROR


def test_python_layer_raises_value_error_for_bad_arguments():
    """before the library is asked: no engine and no GPU are needed to be told"""
    from zlibstream_amd import PNG_RGBA8, PNG_RGBA16, png_compose_batch_device, png_decode_anim_batch
    fr = dict(x=1, y=1, width=2, height=2, dispose_op=0, blend_op=1)
    ok = dict(frame_ptrs=[[4096]], frames=[[fr]], widths=[3], heights=[3], out_ptrs=[8192], format=PNG_RGBA8)
    for change in (dict(widths=[0]), dict(heights=[1 << 31]), dict(out_ptrs=[0]), dict(out_ptrs=[8194]), dict(frame_ptrs=[[0]]), dict(frame_ptrs=[[4098]]),
                   dict(frame_ptrs=[[4096, 4096]]), dict(frames=[[]], frame_ptrs=[[]]), dict(frames=[[dict(fr, x=2)]]), dict(frames=[[dict(fr, height=3)]]),
                   dict(frames=[[dict(fr, x=-1)]]), dict(frames=[[dict(fr, width=0)]]), dict(frames=[[dict(fr, dispose_op=3)]]), dict(frames=[[dict(fr, blend_op=2)]]),
                   dict(format=2), dict(widths=[3, 3]), dict(format=PNG_RGBA16, frame_ptrs=[[4100]])):
        with pytest.raises(ValueError):
            png_compose_batch_device(None, **dict(ok, **change))
    f = png(IDAT)
    for args in (([f], [4096, 8192], [64], PNG_RGBA8), ([f], [0], [64], PNG_RGBA8), ([f], [4100], [64], PNG_RGBA16), ([f], [4096], [-1], PNG_RGBA8),
                 ([f], [4096], [64], 3)):
        with pytest.raises(ValueError):
            png_decode_anim_batch(None, *args)


# ---------------------------------------------------------------- Pillow
def _chunks(f):
    at = 8
    while at < len(f):
        n = struct.unpack(">I", f[at:at + 4])[0]
        yield f[at + 4:at + 8], f[at + 8:at + 8 + n]
        at += 12 + n


def frames_of(f):
    """this library's walk for the frames, and every frame's own pixels: its data chunks taken from the file in order, wrapped
    as a still file of the frame's size and read by Pillow -> (anim, frames with px)"""
    from PIL import Image
    from zlibstream_amd import png_anim_info
    anim, frames = png_anim_info(f)
    data, k = [[] for _ in frames], -1
    for ctype, body in _chunks(f):
        if ctype == b"fcTL":
            k += 1
        elif ctype == b"IDAT" and anim["default_is_frame"]:
            data[0].append(body)
        elif ctype == b"fdAT":
            data[k].append(body[4:])
    for fr, d in zip(frames, data):
        assert (fr["n_chunks"], fr["data_bytes"]) == (len(d), sum(len(x) for x in d))
        still = SIG + ihdr(fr["width"], fr["height"], anim["bit_depth"], anim["color_type"], anim["interlace"]) + chunk(b"IDAT", b"".join(d)) + IEND
        fr["px"] = np.asarray(Image.open(io.BytesIO(still)).convert("RGBA"))
    return anim, frames


def test_the_restatement_agrees_with_pillow_on_source_blended_animations():
    """RGBA animations saved by Pillow with blend 0 and every dispose op, PREVIOUS on frame 0 included (Pillow crops the
    frames to what changed: sub-rectangles).  Pillow's OVER arithmetic is not the specification's: SOURCE only."""
    pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.default_rng(8301)
    seen_dispose, seen_sub = set(), 0
    for case in range(20):
        w, h, n = int(rng.integers(1, 20)), int(rng.integers(1, 12)), int(rng.integers(2, 7))
        imgs = []
        for k in range(n):
            a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            a[..., 3] = np.where(rng.random((h, w)) < 0.3, 0, a[..., 3])
            if k and case % 2:  # most of the frame stays: Pillow writes a small region
                keep = rng.random((h, w)) < 0.8
                a[keep] = np.asarray(imgs[-1])[keep]
            imgs.append(Image.fromarray(a, "RGBA"))
        disposal = [int(rng.integers(0, 3)) for _ in range(n)]
        if case % 5 == 0:
            disposal[0] = PREVIOUS
        b = io.BytesIO()
        imgs[0].save(b, "PNG", save_all=True, append_images=imgs[1:], disposal=disposal, blend=0, duration=40)
        f = b.getvalue()
        anim, frames = frames_of(f)
        assert anim["animated"] == 1 and all(fr["blend_op"] == SOURCE for fr in frames)
        seen_dispose |= {(k == 0, fr["dispose_op"]) for k, fr in enumerate(frames)}
        seen_sub += sum(1 for fr in frames if (fr["width"], fr["height"]) != (w, h))
        shown = compose_ref(w, h, frames, RGBA8)
        back = Image.open(io.BytesIO(f))
        assert back.n_frames == anim["n_frames"] == len(shown)
        for k in range(back.n_frames):
            back.seek(k)
            assert back.convert("RGBA").tobytes() == shown[k], (case, k, disposal)
    assert {d for _, d in seen_dispose} == {NONE, BACKGROUND, PREVIOUS} and (True, PREVIOUS) in seen_dispose and seen_sub > 0
