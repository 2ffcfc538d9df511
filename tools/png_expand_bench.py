"""The expansion of raw PNG scanlines to RGBA on the device (zs_png_expand_batch_device, KX), and what it adds to a whole decode.

    expand        8 images of 2048 x 2048 at (color type, bit depth) (3, 8), (2, 8), (0, 1) and (6, 16), to RGBA8 and to RGBA16:
                  the KX launch alone by device events (zs_ctx_stage_ms "png_expand"), and beside it a plain device-to-device
                  copy of as many bytes as KX writes, by device events as well.  The copy reads B bytes and writes B; KX reads at
                  most B and writes B: a KX much slower than the copy is bound by instruction issue or by its access pattern, not
                  by bandwidth.
    decode        zs_png_decode_files_rgba_batch against zs_png_decode_files_batch on the same 8 files of each type (zlib level 1
                  streams of noisy gradients, filter type Up): wall-clock milliseconds around calls that end in their own wait for
                  the stream; the difference is the expansion with its upload of descriptors and its extra wait.

Every leg is warmed up once, then the legs of a pair alternate --runs times: median and spread (max - min).

    python tools/png_expand_bench.py [--runs 7] [--out profiles/png_expand.log]
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TYPES = ((3, 8), (2, 8), (0, 1), (6, 16))
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def noisy_gradient(row_bytes, height, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    grad = (np.add.outer(np.arange(height) * 3, np.arange(row_bytes)) % 253).astype(np.uint8)
    return (grad + rng.integers(0, 4, grad.shape, dtype=np.uint8)).astype(np.uint8)


def chunk(ctype, data):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data))


def png_file(rows, side, color, depth, plte, trns):
    import numpy as np
    up = rows.copy()
    up[1:] -= rows[:-1]  # filter type Up (uint8 wraps)
    payload = np.concatenate([np.full((side, 1), 2, dtype=np.uint8), up], axis=1).tobytes()
    extra = (chunk(b"PLTE", plte) if plte else b"") + (chunk(b"tRNS", trns) if trns else b"")
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", side, side, depth, color, 0, 0, 0)) + extra +
            chunk(b"IDAT", zlib.compress(payload, 1)) + chunk(b"IEND", b""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_expand.log"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from zlibstream_amd import Engine, PNG_RGBA8, PNG_RGBA16, png_decode_files_batch, png_decode_files_rgba_batch, png_expand_batch_device
    if not torch.cuda.is_available():
        sys.exit("png_expand_bench: no GPU (there is nothing to measure without one)")
    eng = Engine(0)
    n, side = a.images, a.side
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}

    rng = np.random.default_rng(42)
    plte, trns = bytes(rng.integers(0, 256, 768, dtype=np.uint8)), bytes(rng.integers(0, 256, 256, dtype=np.uint8))
    images = {}
    for color, depth in TYPES:
        rb = (side * depth * CHANNELS[color] + 7) // 8
        images[color, depth] = [noisy_gradient(rb, side, 100 * color + depth + i) for i in range(n)]

    # ---------------------------------------------------------------- KX alone, beside a copy of its output bytes
    for color, depth in TYPES:
        raw = images[color, depth]
        d_in = [torch.from_numpy(x.reshape(-1)).cuda() for x in raw]
        in_bytes = sum(x.size for x in raw)
        for fmt, name in ((PNG_RGBA8, "RGBA8"), (PNG_RGBA16, "RGBA16")):
            px = 8 if fmt == PNG_RGBA16 else 4
            out_bytes = n * side * side * px
            d_out = [torch.empty(side * side * px, dtype=torch.uint8, device="cuda") for _ in range(n)]
            src, dst = torch.empty(out_bytes, dtype=torch.uint8, device="cuda").fill_(7), torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            args = ([t.data_ptr() for t in d_in], [side] * n, [side] * n, [depth] * n, [color] * n, [t.data_ptr() for t in d_out])
            kw = dict(plte=[plte if color == 3 else None] * n, trns=[trns if color == 3 else None] * n, format=fmt)

            def kx():
                png_expand_batch_device(eng, *args, **kw)
                return eng.stage_ms()["png_expand"]

            def copy():
                e0.record()
                dst.copy_(src)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)

            torch.cuda.synchronize()
            eng.set_profiling(True)
            kx(), copy()
            t_kx, t_cp = [], []
            for _ in range(a.runs):
                t_kx.append(kx())
                t_cp.append(copy())
            eng.set_profiling(False)
            mk, mc = statistics.median(t_kx), statistics.median(t_cp)
            emit({"leg": "expand", "color_type": color, "bit_depth": depth, "format": name, "images": n, "side": side, "in_bytes": in_bytes, "out_bytes": out_bytes,
                  "kx (device events)": stats(t_kx), "copy of out_bytes (device events)": stats(t_cp),
                  "kx GBps read+written": round((in_bytes + out_bytes) / mk / 1e6, 1), "kx GBps written": round(out_bytes / mk / 1e6, 1),
                  "copy GBps read+written": round(2 * out_bytes / mc / 1e6, 1), "kx over copy": round(mk / mc, 3)})
            del d_out, src, dst
        del d_in

    # ---------------------------------------------------------------- what the expansion adds to a whole decode
    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3  # (both calls return after their own wait for the stream)

    for color, depth in TYPES:
        files = [png_file(x, side, color, depth, plte if color == 3 else b"", trns if color == 3 else b"") for x in images[color, depth]]
        raw_bytes = images[color, depth][0].size
        d_raw = [torch.empty(raw_bytes, dtype=torch.uint8, device="cuda") for _ in range(n)]
        for fmt, name in ((PNG_RGBA8, "RGBA8"), (PNG_RGBA16, "RGBA16")):
            px = 8 if fmt == PNG_RGBA16 else 4
            d_out = [torch.empty(side * side * px, dtype=torch.uint8, device="cuda") for _ in range(n)]

            def raw_call():
                st, _ = png_decode_files_batch(eng, files, [t.data_ptr() for t in d_raw], [raw_bytes] * n)
                assert st == [0] * n, eng.last_error()

            def rgba_call():
                st, _ = png_decode_files_rgba_batch(eng, files, [t.data_ptr() for t in d_out], [side * side * px] * n, format=fmt)
                assert st == [0] * n, eng.last_error()

            timed(raw_call), timed(rgba_call)
            t_raw, t_rgba = [], []
            for _ in range(a.runs):
                t_raw.append(timed(raw_call))
                t_rgba.append(timed(rgba_call))
            assert d_raw[0].cpu().numpy().tobytes() == images[color, depth][0].tobytes()
            mr, mx = statistics.median(t_raw), statistics.median(t_rgba)
            emit({"leg": "decode", "color_type": color, "bit_depth": depth, "format": name, "images": n, "side": side, "file_bytes": sum(len(f) for f in files),
                  "raw_bytes": n * raw_bytes, "rgba_bytes": n * side * side * px, "files to raw scanlines": stats(t_raw), "files to rgba": stats(t_rgba),
                  "expansion adds ms (medians)": round(mx - mr, 4), "share of the raw decode": round((mx - mr) / mr, 4)})
            del d_out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
