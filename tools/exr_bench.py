#!/usr/bin/env python3
"""The OpenEXR calls on one MI355X beside the calls they are built on.  Eight frames of 2048 x 1080 RGBA half, ZIP (16 lines a
chunk, 68 chunks a frame), encoded by one zs_exr_encode_batch_device call and decoded by one zs_exr_decode_files_batch call;
beside each, zs_deflate_batch_device and zs_inflate_batch_device alone on the very same chunks (the predicted bytes, and the
streams of the files that were written, resident on the device); then KE alone, both directions, over the frames' chunks
(zs_exr_unpredict_batch_device, zs_exr_predict_batch_device: the reduce launch and the scan, or the forward kernel), and KT's
predictor-2 kernel (zs_tiff_unpredict_batch_device, 16-bit samples, 4 a pixel) on the same byte count.  The yardsticks are the
existing calls, not KE itself.
Every figure is the median of --repeats timed calls behind a warm-up call, the variants of a group taken in turn inside every
repeat so that a drift of the machine meets all of them; the spread (min .. max) stands beside it.  A host clock around calls
that synchronise their stream.
usage: python tools/exr_bench.py [--frames 8] [--width 2048] [--height 1080] [--repeats 7] [--level 6]
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
from zlibstream_amd import (Engine, deflate_bound, exr_bound, exr_decode_files, exr_encode, exr_file_info, exr_predict, exr_unpredict,  # noqa: E402
                            tiff_unpredict)

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--width", type=int, default=2048)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--level", type=int, default=6)
a = ap.parse_args()
eng = Engine(0)
W, H, N = a.width, a.height, a.frames
CHANNELS = [("A", 1), ("B", 1), ("G", 1), ("R", 1)]


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


def frame(seed):
    """Four half planes of a smooth picture with a little noise, as a renderer leaves it; A is 1.0 almost everywhere."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.sin(x / 97.0 + seed) * np.cos(y / 131.0) + np.sin((x + y) / 411.0)
    planes = [np.ones((H, W), np.float32)] + [base * (0.5 + 0.1 * c) + 0.5 + 0.01 * rng.standard_normal((H, W), dtype=np.float32) for c in range(3)]
    return np.concatenate([p.astype("<f2").view(np.uint8).reshape(-1) for p in planes])  # (W * H * 2 is a multiple of 16: no padding)


assert (W * H * 2) % 16 == 0
frames = [frame(s) for s in range(N)]
raw_bytes = sum(f.size for f in frames)
d_planes = [torch.from_numpy(f).cuda() for f in frames]
images = [dict(planes=d.data_ptr(), width=W, height=H, channels=CHANNELS) for d in d_planes]
bounds = [exr_bound(im) for im in images]
d_files = [torch.empty(b, dtype=torch.uint8, device="cuda") for b in bounds]
rc, lens, _ = exr_encode(eng, images, [d.data_ptr() for d in d_files], bounds, level=a.level)
assert rc == 0
files = [d[:n].cpu().numpy().tobytes() for d, n in zip(d_files, lens)]
d_out = [torch.empty(f.size, dtype=torch.uint8, device="cuda") for f in frames]
rc, _, _, status = exr_decode_files(eng, files, [d.data_ptr() for d in d_out], [f.size for f in frames])
assert rc == 0 and all(torch.equal(o, p) for o, p in zip(d_out, d_planes)), "decode of encode is not the identity"

# the very same chunks for the raw calls: every chunk's predicted bytes, and its stream, back to back on the device
chunks = [(k, c) for k, f in enumerate(files) for c in exr_file_info(f)[2]]
sizes = [c["raw_len"] for _, c in chunks]
at = np.concatenate([[0], np.cumsum([(s + 255) // 256 * 256 for s in sizes])]).astype(np.int64)
d_raw = torch.empty(int(at[-1]), dtype=torch.uint8, device="cuda")  # the chunks' raw bytes: rows of A, B, G, R
for (k, c), o in zip(chunks, at):
    rows = frames[k].reshape(4, H, W * 2)[:, c["y"]:c["y"] + c["h"]].transpose(1, 0, 2).reshape(-1)
    d_raw[int(o):int(o) + rows.size] = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
d_pred, d_back = torch.empty_like(d_raw), torch.empty_like(d_raw)
raw_ptrs, pred_ptrs, back_ptrs = ([d.data_ptr() + int(o) for o in at[:-1]] for d in (d_raw, d_pred, d_back))
exr_predict(eng, raw_ptrs, pred_ptrs, sizes)
z_sizes = [c["data_len"] for _, c in chunks]
z_at = np.concatenate([[0], np.cumsum([(s + 255) // 256 * 256 for s in z_sizes])]).astype(np.int64)
d_z = torch.empty(int(z_at[-1]), dtype=torch.uint8, device="cuda")
for (k, c), o in zip(chunks, z_at):
    d_z[int(o):int(o) + c["data_len"]] = torch.from_numpy(np.frombuffer(files[k], np.uint8, c["data_len"], c["off"]).copy()).cuda()
z_ptrs = [d_z.data_ptr() + int(o) for o in z_at[:-1]]
zcaps = [deflate_bound(s) for s in sizes]
zo_at = np.concatenate([[0], np.cumsum([(s + 255) // 256 * 256 for s in zcaps])]).astype(np.int64)
d_zo = torch.empty(int(zo_at[-1]), dtype=torch.uint8, device="cuda")
zo_ptrs = [d_zo.data_ptr() + int(o) for o in zo_at[:-1]]
zlib_chunks = [i for i, (_, c) in enumerate(chunks) if c["data_len"] < c["raw_len"]]  # (a chunk stored raw is no stream)
stored_raw = len(chunks) - len(zlib_chunks)

head = {"frames": N, "width": W, "height": H, "chunks": len(chunks), "raw_mib": round(raw_bytes / 2**20, 1), "file_mib": round(sum(lens) / 2**20, 1),
        "chunks_stored_raw": stored_raw, "level": a.level}
print(json.dumps({"group": "setup", **head}), flush=True)

t = timed({
    "exr_encode": lambda: exr_encode(eng, images, [d.data_ptr() for d in d_files], bounds, level=a.level),
    "deflate_alone": lambda: eng.deflate_batch_device(pred_ptrs, sizes, zo_ptrs, zcaps, level=a.level),
    "ke_forward_alone": lambda: exr_predict(eng, raw_ptrs, pred_ptrs, sizes),
})
print(json.dumps({"group": "encode", **t}), flush=True)

t = timed({
    "exr_decode_files": lambda: exr_decode_files(eng, files, [d.data_ptr() for d in d_out], [f.size for f in frames]),
    "inflate_alone": lambda: eng.inflate_batch_device([z_ptrs[i] for i in zlib_chunks], [z_sizes[i] for i in zlib_chunks], [back_ptrs[i] for i in zlib_chunks],
                                                      [sizes[i] for i in zlib_chunks]),
    "ke_undo_alone": lambda: exr_unpredict(eng, pred_ptrs, back_ptrs, sizes),
})
print(json.dumps({"group": "decode", **t}), flush=True)

# KE beside KT on equal bytes: one chunk a frame-sized strip set, 16-bit samples, 4 a pixel, predictor 2
n = len(chunks)
kt = timed({
    "ke_undo": lambda: exr_unpredict(eng, pred_ptrs, back_ptrs, sizes),
    "ke_forward": lambda: exr_predict(eng, raw_ptrs, pred_ptrs, sizes),
    "kt_undo_predictor2": lambda: tiff_unpredict(eng, pred_ptrs, back_ptrs, [W] * n, [s // (W * 8) for s in sizes], [16] * n, [4] * n, [2] * n),
})
for k, v in kt.items():
    v["gb_per_s_read_plus_written"] = round(2 * sum(sizes) / (v["ms_median"] * 1e-3) / 1e9, 1)
print(json.dumps({"group": "kernels", "bytes": sum(sizes), **kt}), flush=True)
