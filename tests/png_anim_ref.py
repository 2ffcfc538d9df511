"""Animated PNG for the tests: chunk builders for hand-built files, and the numpy restatement of the compose rules of
include/zsgpu.h (zs_png_compose_batch_device) -- frame by frame on a full canvas, the APNG specification's integer OVER with
divisions on int64 arrays.  tests/test_png_anim_host.py anchors the restatement to Pillow's own frame-by-frame decode; the GPU
tests compare the device's bytes with it."""
import struct
import zlib

import numpy as np

from test_gpu_png_expand import ADAM7, CHANNELS, _filtered, _pack, _unpack  # noqa: F401  (the still files' builders: no GPU is touched by the import)

SIG = b"\x89PNG\r\n\x1a\n"
RGBA8, RGBA16 = 0, 1
NONE, BACKGROUND, PREVIOUS = 0, 1, 2
SOURCE, OVER = 0, 1


# ---------------------------------------------------------------- chunks
def chunk(ctype, data, crc=None):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data) if crc is None else crc)


def flipped(ctype, data):
    return chunk(ctype, data, crc=zlib.crc32(ctype + data) ^ 0x10)


def ihdr(w, h, depth=8, color=6, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color, 0, 0, interlace))


def actl(n_frames, n_plays=0):
    return chunk(b"acTL", struct.pack(">II", n_frames, n_plays))


def fctl_data(seq, w, h, x=0, y=0, delay_num=1, delay_den=10, dispose=NONE, blend=SOURCE):
    return struct.pack(">IIIIIHHBB", seq, w, h, x, y, delay_num, delay_den, dispose, blend)


def fctl(seq, w, h, **kw):
    return chunk(b"fcTL", fctl_data(seq, w, h, **kw))


def fdat(seq, data):
    return chunk(b"fdAT", struct.pack(">I", seq) + data)


IEND = chunk(b"IEND", b"")


# ---------------------------------------------------------------- scanlines to a frame's zlib stream
def frame_stream(rows, w, bits, interlace, k=0):
    """(h, row_bytes) raw scanlines of one frame (padding bits zero) -> its zlib stream, Adam7 passes where interlace is 1"""
    if interlace:
        px, payload = _unpack(rows, w, bits), b""
        for xs, ys, xst, yst in ADAM7:
            sub = px[ys::yst, xs::xst]
            if sub.shape[0] and sub.shape[1]:
                payload += _filtered(_pack(sub, bits), k)
    else:
        payload = _filtered(rows, k)
    return zlib.compress(payload, 0 if k % 3 == 0 else 6)


def build_apng(w, h, depth, color, interlace, frames, default_stream=None, before=(), n_plays=0, cuts=2, between=b""):
    """A whole animated file.  frames: dicts of x, y, width, height, dispose_op, blend_op and stream (the frame's zlib stream).
    default_stream None: frame 0 is the default image (it must be the whole canvas) and its stream goes into the IDAT chunks;
    otherwise default_stream does, and every frame is fdAT.  Every stream is cut into `cuts` chunks, `between` (whole chunks)
    between them."""
    out = SIG + ihdr(w, h, depth, color, interlace) + b"".join(before) + actl(len(frames), n_plays)
    seq = 0

    def pieces(s):
        step = max(1, -(-len(s) // cuts))
        return [s[i:i + step] for i in range(0, len(s), step)] or [b""]

    def fc(f):
        nonlocal seq
        seq += 1
        return fctl(seq - 1, f["width"], f["height"], x=f["x"], y=f["y"], delay_num=f.get("delay_num", 1), delay_den=f.get("delay_den", 10),
                    dispose=f["dispose_op"], blend=f["blend_op"])

    rest = list(frames)
    if default_stream is None:
        out += fc(rest[0]) + b"".join(chunk(b"IDAT", p) for p in pieces(rest[0]["stream"]))
        rest = rest[1:]
    else:
        out += b"".join(chunk(b"IDAT", p) for p in pieces(default_stream))
    for f in rest:
        out += fc(f)
        parts = []
        for p in pieces(f["stream"]):
            parts.append(fdat(seq, p))
            seq += 1
        out += between.join(parts)
    return out + IEND


# ---------------------------------------------------------------- the compose rules, restated
def over_ref(fg, bg, top):
    """(..., 4) int64 arrays: foreground over canvas, the APNG specification's sample code with integers"""
    fa, ba = fg[..., 3:4], bg[..., 3:4]
    u, v = fa * top, (top - fa) * ba
    al = u + v
    safe = np.where(al == 0, 1, al)
    mixed = np.concatenate([(fg[..., :3] * u + bg[..., :3] * v) // safe, al // top], axis=-1)
    return np.where(fa == 0, bg, np.where((fa == top) | (ba == 0), fg, mixed))


def compose_ref(w, h, frames, fmt):
    """frames: dicts of x, y, width, height, dispose_op, blend_op and px, a (height, width, 4) array of the frame's own
    pixels -> one bytes object per canvas: what a viewer shows while that frame is up"""
    top = 65535 if fmt == RGBA16 else 255
    canvas = np.zeros((h, w, 4), dtype=np.int64)  # transparent black
    shown = []
    for k, f in enumerate(frames):
        region = (slice(f["y"], f["y"] + f["height"]), slice(f["x"], f["x"] + f["width"]))
        previous = canvas[region].copy()
        px = np.asarray(f["px"]).astype(np.int64).reshape(f["height"], f["width"], 4)
        canvas[region] = px if f["blend_op"] == SOURCE else over_ref(px, canvas[region], top)
        assert canvas.min() >= 0 and canvas.max() <= top
        shown.append(canvas.astype("<u2" if fmt == RGBA16 else np.uint8).tobytes())
        if f["dispose_op"] == BACKGROUND or (f["dispose_op"] == PREVIOUS and k == 0):
            canvas[region] = 0
        elif f["dispose_op"] == PREVIOUS:
            canvas[region] = previous
    return shown
