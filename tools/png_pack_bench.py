"""The pack of RGBA pixels into raw PNG scanlines (zs_png_pack_batch_device, KG), the survey in front of it
(zs_png_survey_batch_device, KV), and what the two add to a whole encode.

    pack          8 images of 2048 x 2048 whose pixels are the expansion (KX) of noisy scanlines at (color type, bit depth) (3, 8),
                  (2, 8), (0, 1), (6, 8) -- RGBA8 -- and (6, 16) -- RGBA16: the KG launch back to that pair, the two KV launches
                  and the KX launch that made the pixels, each alone by device events (zs_ctx_stage_ms "png_pack", "png_survey",
                  "png_expand"), and beside them a plain device-to-device copy of as many bytes as KG reads, by device events as
                  well.  KG and KV read B bytes and write at most B; the copy reads B and writes B: a KG or KV much slower than
                  the copy is bound by instruction issue or by its access pattern, not by bandwidth.
    encode        zs_png_encode_rgba_batch_device on those pixels against zs_png_encode_interlace_batch_device on scanlines packed
                  beforehand (the pair and the palette the first call chose): wall-clock milliseconds around calls that end in
                  their own wait for the stream; the difference is what the new front end costs -- survey, choice, pack, and
                  their three waits.

Every leg is warmed up once, then the legs alternate --runs times: median and spread (max - min).

    python tools/png_pack_bench.py [--runs 7] [--out profiles/png_pack.log]
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

TYPES = ((3, 8), (2, 8), (0, 1), (6, 16), (6, 8))
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def noisy_gradient(row_bytes, height, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    grad = (np.add.outer(np.arange(height) * 3, np.arange(row_bytes)) % 253).astype(np.uint8)
    return (grad + rng.integers(0, 4, grad.shape, dtype=np.uint8)).astype(np.uint8)


def chunk(ctype, data):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_pack.log"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from zlibstream_amd import (Engine, PNG_RGBA8, PNG_RGBA16, deflate_bound, png_encode_interlace_batch_device, png_encode_rgba_batch_device,
                                png_expand_batch_device, png_file_bound, png_idat_layout, png_pack_batch_device, png_survey_batch_device)
    if not torch.cuda.is_available():
        sys.exit("png_pack_bench: no GPU (there is nothing to measure without one)")
    eng = Engine(0)
    n, side = a.images, a.side
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3  # (the calls return after their own wait for the stream)

    rng = np.random.default_rng(42)
    # a palette of 256 different colours, so that the survey finds them all again
    rgb = rng.choice(1 << 24, size=256, replace=False).astype(np.uint32)
    plte = np.stack([rgb & 255, rgb >> 8 & 255, rgb >> 16], axis=1).astype(np.uint8).tobytes()
    trns = bytes(rng.integers(0, 256, 256, dtype=np.uint8))
    for color, depth in TYPES:
        fmt, name = (PNG_RGBA16, "RGBA16") if depth == 16 else (PNG_RGBA8, "RGBA8")
        px = 8 if fmt == PNG_RGBA16 else 4
        rb = (side * depth * CHANNELS[color] + 7) // 8
        raw = [noisy_gradient(rb, side, 100 * color + depth + i) for i in range(n)]
        d_raw = [torch.from_numpy(x.reshape(-1)).cuda() for x in raw]
        d_px = [torch.empty(side * side * px, dtype=torch.uint8, device="cuda") for _ in range(n)]
        d_back = [torch.empty(rb * side, dtype=torch.uint8, device="cuda") for _ in range(n)]
        raw_bytes, px_bytes = n * rb * side, n * side * side * px
        src, dst = torch.empty(px_bytes, dtype=torch.uint8, device="cuda").fill_(7), torch.empty(px_bytes, dtype=torch.uint8, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dims = ([side] * n, [side] * n)
        kw = dict(plte=[plte if color == 3 else None] * n, trns=[trns if color == 3 else None] * n, format=fmt)

        def kx():
            png_expand_batch_device(eng, [t.data_ptr() for t in d_raw], *dims, [depth] * n, [color] * n, [t.data_ptr() for t in d_px], **kw)
            return eng.stage_ms()["png_expand"]

        def kg():
            png_pack_batch_device(eng, [t.data_ptr() for t in d_px], *dims, [depth] * n, [color] * n, [t.data_ptr() for t in d_back], **kw)
            return eng.stage_ms()["png_pack"]

        def kv():
            png_survey_batch_device(eng, [t.data_ptr() for t in d_px], *dims, format=fmt)
            return eng.stage_ms()["png_survey"]

        def copy():
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        # ------------------------------------------------------------ KG, KV and KX alone, beside a copy of KG's input bytes
        torch.cuda.synchronize()
        eng.set_profiling(True)
        kx(), kg(), kv(), copy()
        assert d_back[0].cpu().numpy().tobytes() == raw[0].tobytes(), "the pack does not return what the expansion was given"
        t = {"kx": [], "kg": [], "kv": [], "copy": []}
        for _ in range(a.runs):
            t["kx"].append(kx()), t["kg"].append(kg()), t["kv"].append(kv()), t["copy"].append(copy())
        eng.set_profiling(False)
        m = {k: statistics.median(v) for k, v in t.items()}
        emit({"leg": "pack", "color_type": color, "bit_depth": depth, "format": name, "images": n, "side": side, "rgba_bytes": px_bytes, "raw_bytes": raw_bytes,
              "kg (device events)": stats(t["kg"]), "kv, both launches (device events)": stats(t["kv"]), "kx (device events)": stats(t["kx"]),
              "copy of rgba_bytes (device events)": stats(t["copy"]), "kg GBps read": round(px_bytes / m["kg"] / 1e6, 1),
              "kv GBps read": round(px_bytes / m["kv"] / 1e6, 1), "copy GBps read+written": round(2 * px_bytes / m["copy"] / 1e6, 1),
              "kg over copy": round(m["kg"] / m["copy"], 3), "kv over copy": round(m["kv"] / m["copy"], 3), "kx over copy": round(m["kx"] / m["copy"], 3)})
        del src, dst

        # ------------------------------------------------------------ what the front end adds to a whole encode
        cap = png_file_bound(deflate_bound(png_idat_layout(side, side, 8 * px, 0)[0]), 0, 1048)
        d_out = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
        ptrs = dict(px=[t.data_ptr() for t in d_px], out=[t.data_ptr() for t in d_out], back=[t.data_ptr() for t in d_back])
        lens, cts, bds = png_encode_rgba_batch_device(eng, ptrs["px"], *dims, [2] * n, ptrs["out"], [cap] * n, format=fmt, level=a.level)
        first = d_out[0][:lens[0]].cpu().numpy().tobytes()
        # the scanlines packed beforehand, at the pair and with the palette that call chose
        surveys = png_survey_batch_device(eng, ptrs["px"], *dims, format=fmt)
        plte2 = [b"".join(bytes(c[:3]) for c in s["colors"]) if ct == 3 else None for s, ct in zip(surveys, cts)]
        trns2 = [bytes(c[3] for c in s["colors"]).rstrip(b"\xff") or None if ct == 3 else None for s, ct in zip(surveys, cts)]
        extra = [chunk(b"PLTE", p) + (chunk(b"tRNS", t2) if t2 else b"") if p else b"" for p, t2 in zip(plte2, trns2)]
        d_pre = [torch.empty((side * bd * CHANNELS[ct] + 7) // 8 * side, dtype=torch.uint8, device="cuda") for ct, bd in zip(cts, bds)]
        png_pack_batch_device(eng, ptrs["px"], *dims, bds, cts, [t.data_ptr() for t in d_pre], plte=plte2, trns=trns2, format=fmt)

        def rgba_call():
            png_encode_rgba_batch_device(eng, ptrs["px"], *dims, [2] * n, ptrs["out"], [cap] * n, format=fmt, level=a.level)

        def packed_call():
            png_encode_interlace_batch_device(eng, [t.data_ptr() for t in d_pre], *dims, bds, cts, [2] * n, ptrs["out"], [cap] * n, extra=extra, level=a.level)

        timed(packed_call)
        assert d_out[0][:lens[0]].cpu().numpy().tobytes() == first, "the two calls do not write the same file"
        timed(rgba_call)
        t_pre, t_rgba = [], []
        for _ in range(a.runs):
            t_pre.append(timed(packed_call))
            t_rgba.append(timed(rgba_call))
        mp, mr = statistics.median(t_pre), statistics.median(t_rgba)
        emit({"leg": "encode", "wanted": [color, depth], "chosen": sorted(set(zip(cts, bds))), "format": name, "images": n, "side": side, "level": a.level,
              "file_bytes": sum(lens), "rgba_bytes": px_bytes, "packed scanlines to files": stats(t_pre), "rgba to files": stats(t_rgba),
              "front end adds ms (medians)": round(mr - mp, 4), "share of the packed encode": round((mr - mp) / mp, 4)})
        del d_out, d_pre, d_raw, d_px, d_back
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
