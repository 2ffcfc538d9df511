#!/usr/bin/env python3
"""The TIFF calls on one MI355X beside the raw batch calls they are built on.  Three images -- RGB8 in 256 x 256 tiles with
predictor 2, 16-bit gray in strips with predictor 2, float32 in strips with predictor 3 -- each encoded by one
zs_tiff_encode_batch_device call and decoded by one zs_tiff_decode_files_batch call; beside each, zs_deflate_batch_device and
zs_inflate_batch_device on the very same chunks (the predicted bytes, and the streams of the file that was written, resident on
the device).  What the TIFF call costs over the raw one is the predictor launch, the framing copy (encode), and the upload
of the file and the Adler-32 launch of its own (decode).  Then the predictor kernels alone, in GB/s of bytes read plus bytes
written, beside KX (zs_png_expand_batch_device, RGB8 to RGBA8) on an image of the same bytes; and the gray image written with
strips of 64 KiB, 256 KiB and 1 MiB, which is what the default of rows_per_strip = 0 was chosen from.
Every figure is the median of --repeats timed calls behind a warm-up call, the variants of a group taken in turn inside every
repeat so that a drift of the machine meets all of them; the spread (min .. max) stands beside it.  A host clock around calls
that synchronise their stream.
usage: python tools/tiff_calls.py [--side 8192] [--repeats 7] [--level 6]
Prints one JSON line per group; fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from zlibstream_amd import (Engine, deflate_bound, png_expand_batch_device, tiff_bound, tiff_decode_files, tiff_encode, tiff_file_info, tiff_predict,  # noqa: E402
                            tiff_unpredict)

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=8192)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--level", type=int, default=6)
a = ap.parse_args()
eng = Engine(0)


def timed(variants):
    """variants: {name: callable}.  One warm-up call each, then --repeats turns through all of them."""
    for f in variants.values():
        f()
    times = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)} for k, v in times.items()}


def picture(width, height, spp, kind):
    """A smooth picture with a little noise in its low bits, as a camera or a sensor leaves it: rows of little-endian samples."""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:height, 0:width].astype(np.float32)
    base = np.sin(x / 97.0) * np.cos(y / 131.0) + np.sin((x + y) / 411.0)
    planes = [base * (0.5 + 0.1 * c) + 0.02 * rng.standard_normal((height, width), dtype=np.float32) for c in range(spp)]
    v = np.stack(planes, axis=-1)
    if kind == "f4":
        return v.astype("<f4").view(np.uint8).reshape(height, -1)
    top = 255 if kind == "u1" else 65535
    return np.clip((v + 2) / 4 * top, 0, top).astype("<" + kind).view(np.uint8).reshape(height, -1)


def one_image(title, rows, put):
    width, height, raw = put["width"], put["height"], rows.size
    d_pix = torch.from_numpy(rows.reshape(-1)).cuda()
    image = dict(put, pixels=d_pix.data_ptr())
    bound = tiff_bound(image)
    d_file = torch.empty(bound, dtype=torch.uint8, device="cuda")
    rc, lens, _ = tiff_encode(eng, [image], [d_file.data_ptr()], [bound], level=a.level)
    assert rc == 0
    file = d_file[:lens[0]].cpu().numpy().tobytes()
    info, chunks = tiff_file_info(file)
    n = len(chunks)
    spp, bits, predictor = put.get("spp", 1), put.get("bits", 8), put.get("predictor", 1)
    # the very same chunks for the raw calls: the predicted bytes of every chunk, back to back, and the file's streams on the device
    sizes = [(info["chunk_h"] if info["tiled"] else c["h"]) * (info["chunk_w"] * spp * bits // 8) for c in chunks]
    at = np.concatenate([[0], np.cumsum([(s + 255) // 256 * 256 for s in sizes])])
    d_pred = torch.empty(int(at[-1]) + 256, dtype=torch.uint8, device="cuda")
    row_bytes = info["row_bytes"]
    in_ptrs = [d_pix.data_ptr() + c["y"] * row_bytes + c["x"] * spp * bits // 8 for c in chunks]
    pred_ptrs = [d_pred.data_ptr() + int(o) for o in at[:-1]]
    # (the forward kernel reads its rows at the image's pitch only inside zs_tiff_encode_batch_device; alone it takes an image
    # of the part's own width, so the chunks are predicted from their own copies here)
    parts = [np.ascontiguousarray(rows[c["y"]:c["y"] + c["h"], c["x"] * spp * bits // 8:(c["x"] + c["w"]) * spp * bits // 8]) for c in chunks]
    d_parts = [torch.from_numpy(p.reshape(-1)).cuda() for p in parts]
    args = ([t.data_ptr() for t in d_parts], pred_ptrs, [c["w"] for c in chunks], [c["h"] for c in chunks], [bits] * n, [spp] * n, [predictor] * n)
    kw = dict(widths=[info["chunk_w"]] * n, heights=[info["chunk_h"] if info["tiled"] else c["h"] for c in chunks])
    tiff_predict(eng, *args, **kw)
    caps = [deflate_bound(s) for s in sizes]
    zat = np.concatenate([[0], np.cumsum([(c + 255) // 256 * 256 for c in caps])])
    d_zs = torch.empty(int(zat[-1]) + 256, dtype=torch.uint8, device="cuda")
    zs_ptrs = [d_zs.data_ptr() + int(o) for o in zat[:-1]]
    d_file_in = torch.from_numpy(np.frombuffer(file, np.uint8).copy()).cuda()
    d_out = torch.empty(info["out_len"] + 256, dtype=torch.uint8, device="cuda")
    d_raw_out = torch.empty(int(at[-1]) + 256, dtype=torch.uint8, device="cuda")
    d_img = torch.empty(raw + 256, dtype=torch.uint8, device="cuda")
    img_ptrs = [d_img.data_ptr() + c["y"] * row_bytes + c["x"] * spp * bits // 8 for c in chunks]

    def decode():
        rc, _, _, _ = tiff_decode_files(eng, [file], [d_out.data_ptr()], [info["out_len"]])
        assert rc == 0

    enc = timed({"tiff_encode": lambda: tiff_encode(eng, [image], [d_file.data_ptr()], [bound], level=a.level),
                 "deflate_batch_device": lambda: eng.deflate_batch_device(pred_ptrs, sizes, zs_ptrs, caps, level=a.level)})
    dec = timed({"tiff_decode_files": decode,
                 "inflate_batch_device": lambda: eng.inflate_batch_device([d_file_in.data_ptr() + c["off"] for c in chunks], [c["comp_len"] for c in chunks],
                                                                          [d_raw_out.data_ptr() + int(o) for o in at[:-1]], sizes)})
    assert torch.equal(d_out[:raw], d_pix)
    # the kernels alone: chunk -> chunk of the same size (a kernel's traffic is what it reads plus what it writes)
    full = [info["chunk_h"] if info["tiled"] else c["h"] for c in chunks]
    ker = timed({"unpredict": lambda: tiff_unpredict(eng, pred_ptrs, [d_raw_out.data_ptr() + int(o) for o in at[:-1]], [info["chunk_w"]] * n, full, [bits] * n, [spp] * n,
                                                     [predictor] * n),
                 "predict": lambda: tiff_predict(eng, *args, **kw)})
    total = sum(sizes)
    for k in ker:
        ker[k]["GB_per_s"] = round(2 * total / ker[k]["ms_median"] / 1e6, 1)
    for k, v in list(enc.items()) + list(dec.items()):
        v["GB_per_s_raw"] = round(raw / v["ms_median"] / 1e6, 2)
    print(json.dumps({"group": title, "width": width, "height": height, "raw_bytes": raw, "file_bytes": len(file), "chunks": n, "chunk_bytes": sizes[0],
                      "level": a.level, "encode": enc, "decode": dec, "kernels": ker}), flush=True)
    return file


side = a.side
rgb = picture(side, side, 3, "u1")
one_image("rgb8 tiles 256x256 predictor 2", rgb, dict(width=side, height=side, spp=3, photometric=2, predictor=2, tile_width=256, tile_height=256))
# KX on an image of the same bytes: RGB8 rows expanded to RGBA8
d_in = torch.from_numpy(rgb.reshape(-1)).cuda()
d_rgba = torch.empty(side * side * 4, dtype=torch.uint8, device="cuda")
kx = timed({"png_expand (KX)": lambda: png_expand_batch_device(eng, [d_in.data_ptr()], [side], [side], [8], [2], [d_rgba.data_ptr()])})
kx["png_expand (KX)"]["GB_per_s"] = round((rgb.size + side * side * 4) / kx["png_expand (KX)"]["ms_median"] / 1e6, 1)
print(json.dumps({"group": "KX on the same rgb8 bytes", "kernels": kx}), flush=True)
del d_in, d_rgba, rgb
gray = picture(side, side, 1, "u2")
for strip in (64 << 10, 256 << 10, 1 << 20):
    one_image("gray16 strips of %d KiB predictor 2" % (strip >> 10), gray, dict(width=side, height=side, bits=16, predictor=2, rows_per_strip=strip // (2 * side)))
del gray
fl = picture(side // 2, side // 2, 1, "f4")
one_image("float32 strips predictor 3", fl, dict(width=side // 2, height=side // 2, bits=32, sample_format=3, predictor=3))
