"""An animated PNG reader for the tests, independent of the engine: the chunk walk with zlib.crc32 on every chunk,
zlib.decompress, unfiltering (PNG specification 9.2), de-interlacing (8.2) and the expansion and compose restatements of
tests/test_gpu_png_expand.py and tests/png_anim_ref.py; and the frame-diff rule restated on numpy arrays.  The walk asserts
the structure the APNG specification asks of a file whose default image is its first frame."""
import struct
import zlib

import numpy as np

from png_anim_ref import SIG, compose_ref
from test_gpu_png_expand import ADAM7, CHANNELS, _pack, _unpack, expand_ref

RGBA8, RGBA16 = 0, 1


def diff_ref(canvases):
    """canvases: (n_frames, h, w, 4) array -> [(x, y, width, height)]: frame 0 the whole canvas, frame f the smallest rectangle
    that holds every pixel that differs between canvas f - 1 and canvas f, (0, 0, 1, 1) where none does"""
    n, h, w, _ = canvases.shape
    out = [(0, 0, w, h)]
    for f in range(1, n):
        ys, xs = np.nonzero((canvases[f] != canvases[f - 1]).any(axis=2))
        out.append((0, 0, 1, 1) if len(xs) == 0 else (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)))
    return out


def walk(f):
    """-> dict(width, height, depth, color, interlace, plte, trns, types, n_plays, frames); a frame is a dict of x, y, width,
    height, delay_num, delay_den, dispose_op, blend_op, stream and pieces (the stream bytes of each of its chunks)"""
    assert f[:8] == SIG
    chunks, at = [], 8
    while at < len(f):
        n = int.from_bytes(f[at:at + 4], "big")
        ctype, data = f[at + 4:at + 8], f[at + 8:at + 8 + n]
        assert len(data) == n and int.from_bytes(f[at + 8 + n:at + 12 + n], "big") == zlib.crc32(ctype + data), (ctype, at)
        chunks.append((ctype, data))
        at += 12 + n
    assert at == len(f) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    types = [t for t, _ in chunks]
    w, h, depth, color, comp, flt, il = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (comp, flt) == (0, 0) and types.count(b"IHDR") == 1 and types.count(b"IEND") == 1 and types.count(b"PLTE") <= 1 and types.count(b"tRNS") <= 1
    out = dict(width=w, height=h, depth=depth, color=color, interlace=il, plte=dict(chunks).get(b"PLTE", b""), trns=dict(chunks).get(b"tRNS", b""), types=types,
               n_plays=None, frames=[])
    if b"acTL" not in types:  # a still image: one frame, the IDAT stream
        assert b"fcTL" not in types and b"fdAT" not in types
        pieces = [d for t, d in chunks if t == b"IDAT"]
        out["frames"].append(dict(x=0, y=0, width=w, height=h, delay_num=None, delay_den=None, dispose_op=0, blend_op=0, stream=b"".join(pieces), pieces=pieces))
        return out
    assert types.count(b"acTL") == 1 and types.index(b"acTL") < types.index(b"IDAT")
    n_frames, out["n_plays"] = struct.unpack(">II", dict(chunks)[b"acTL"])
    seq, idat_seen, idat_over = 0, False, False
    for ctype, data in chunks:
        if ctype == b"fcTL":
            s, fw, fh, x, y, dn, dd, dispose, blend = struct.unpack(">IIIIIHHBB", data)
            assert s == seq, "fcTL sequence number %d, not %d" % (s, seq)
            seq += 1
            assert not out["frames"] or out["frames"][-1]["pieces"], "an fcTL without frame data"
            out["frames"].append(dict(x=x, y=y, width=fw, height=fh, delay_num=dn, delay_den=dd, dispose_op=dispose, blend_op=blend, pieces=[]))
            idat_over = idat_seen
        elif ctype == b"IDAT":
            assert len(out["frames"]) == 1 and not idat_over, "IDAT is frame 0's data: one fcTL in front of it, the chunks consecutive"
            idat_seen = True
            out["frames"][0]["pieces"].append(data)
        elif ctype == b"fdAT":
            assert idat_seen and len(out["frames"]) >= 2 and int.from_bytes(data[:4], "big") == seq, "fdAT sequence number"
            seq += 1
            out["frames"][-1]["pieces"].append(data[4:])
    assert len(out["frames"]) == n_frames and all(fr["pieces"] for fr in out["frames"])
    f0 = out["frames"][0]
    assert (f0["x"], f0["y"], f0["width"], f0["height"]) == (0, 0, w, h)
    for fr in out["frames"]:
        fr["stream"] = b"".join(fr["pieces"])
        assert fr["x"] + fr["width"] <= w and fr["y"] + fr["height"] <= h and fr["width"] >= 1 and fr["height"] >= 1
    return out


def unfilter(data, rb, h, bpp):
    """h rows of (filter type, rb filtered bytes) -> (h, rb) uint8, PNG specification 9.2; bpp: bytes per complete pixel, at least 1"""
    assert len(data) == h * (rb + 1)
    out = np.zeros((h, rb), dtype=np.uint8)
    prev = [0] * rb
    for y in range(h):
        ft, line = data[y * (rb + 1)], data[y * (rb + 1) + 1:(y + 1) * (rb + 1)]
        assert ft <= 4
        cur = [0] * rb
        for i in range(rb):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if ft == 0:
                p = 0
            elif ft == 1:
                p = a
            elif ft == 2:
                p = b
            elif ft == 3:
                p = (a + b) // 2
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                p = a if pa <= pb and pa <= pc else b if pb <= pc else c
            cur[i] = (line[i] + p) & 255
        out[y] = cur
        prev = cur
    return out


def scanlines(stream, w, h, bits, interlace):
    """a frame's zlib stream -> its (h, row_bytes) raw scanlines"""
    data = zlib.decompress(stream)
    bpp = max(1, bits // 8)
    if not interlace:
        return unfilter(data, (w * bits + 7) // 8, h, bpp)
    px = np.zeros((h, w) if bits < 8 else (h, w, bits // 8), dtype=np.uint8)
    at = 0
    for xs, ys, xst, yst in ADAM7:
        pw, ph = (w - xs + xst - 1) // xst, (h - ys + yst - 1) // yst
        if pw <= 0 or ph <= 0:
            continue
        rb = (pw * bits + 7) // 8
        rows = unfilter(data[at:at + ph * (rb + 1)], rb, ph, bpp)
        at += ph * (rb + 1)
        px[ys::yst, xs::xst] = _unpack(rows, pw, bits)
    assert at == len(data), "the stream holds bytes beyond its passes"
    return _pack(px, bits)


def canvases_of(f, fmt):
    """a file -> (its walk, one bytes object per canvas), every frame decoded here and composed by png_anim_ref.compose_ref"""
    a = walk(f)
    bits = a["depth"] * CHANNELS[a["color"]]
    frames = []
    for fr in a["frames"]:
        rows = scanlines(fr["stream"], fr["width"], fr["height"], bits, a["interlace"])
        px = expand_ref(rows, fr["width"], a["color"], a["depth"], a["plte"], a["trns"], fmt)
        frames.append(dict(fr, px=np.frombuffer(px, dtype="<u2" if fmt == RGBA16 else np.uint8).reshape(fr["height"], fr["width"], 4)))
    return a, compose_ref(a["width"], a["height"], frames, fmt)
