"""Animated PNG: the compose launch (zs_png_compose_batch_device, KM) beside the expansion (KX) that feeds it, and a whole
zs_png_decode_anim_batch call.

    compose       frames of random RGBA8 pixels on the device (a third transparent, a third opaque) -> canvases, by device
                  events (zs_ctx_stage_ms "png_compose"), twice: every frame SOURCE / NONE ("source"), and the six dispose-blend
                  pairs in turn ("mixed", where a third of the OVER pixels take the divisions).  GB/s counts the canvas bytes
                  written plus the region bytes read.  Beside it KX ("png_expand") in the same run on as many images of the
                  canvas size as the animations have frames, colour type 6 at 8 bits to RGBA8 (bytes read plus bytes written):
                  both kernels stream, so KX is the yardstick.
    files         zs_png_decode_anim_batch on files of those frames (every frame the same compressed noisy gradient, so that
                  building them costs nothing): wall-clock milliseconds around a call that ends in its own wait for the
                  stream, and the stages it reports.

The cases: one 1024 x 1024 animation of 64 whole-canvas frames; one of 64 frames of 64 x 64 on a grid; 256 animations of
128 x 128 with 16 whole-canvas frames each.  Every leg is warmed up once, then the legs alternate --runs times: median and
spread (max - min).

    python tools/png_anim_bench.py [--runs 7] [--out profiles/png_anim.log]
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

SIG = b"\x89PNG\r\n\x1a\n"
PAIRS = [(d, b) for d in (0, 1, 2) for b in (0, 1)]


def chunk(ctype, data):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data))


def build_file(w, h, frames, streams):
    """RGBA8, not interlaced, the default image frame 0 when it is the whole canvas (else a default image of its own)"""
    out = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"acTL", struct.pack(">II", len(frames), 0))
    seq = 0
    first_is_default = (frames[0]["x"], frames[0]["y"], frames[0]["width"], frames[0]["height"]) == (0, 0, w, h)
    if not first_is_default:
        out += chunk(b"IDAT", zlib.compress(bytes(h * (w * 4 + 1)), 1))
    for k, (f, s) in enumerate(zip(frames, streams)):
        out += chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, f["width"], f["height"], f["x"], f["y"], 1, 30, f["dispose_op"], f["blend_op"]))
        seq += 1
        if k == 0 and first_is_default:
            out += chunk(b"IDAT", s)
        else:
            out += chunk(b"fdAT", struct.pack(">I", seq) + s)
            seq += 1
    return out + chunk(b"IEND", b"")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--scale", type=int, default=1, help="divide the canvases' sides by this (a rehearsal; 1 for the log)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_anim.log"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from zlibstream_amd import Engine, PNG_RGBA8, png_compose_batch_device, png_decode_anim_batch, png_expand_batch_device
    if not torch.cuda.is_available():
        sys.exit("png_anim_bench: no GPU (there is nothing to measure without one)")
    eng = Engine(0)
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}

    big, small, cell = 1024 // a.scale, 128 // a.scale, 64 // a.scale
    grid = big // cell
    cases = (("1 animation, 64 whole-canvas frames", 1, big, [(0, 0, big, big)] * 64),
             ("1 animation, 64 frames of a 16th of the side", 1, big, [((k % grid) * cell, (k * 5 % grid) * cell, cell, cell) for k in range(64)]),
             ("256 animations, 16 whole-canvas frames", 256, small, [(0, 0, small, small)] * 16))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for name, n_anim, side, regions in cases:
        n_fr = len(regions)
        canvas = side * side * 4
        region_bytes = sum(w * h * 4 for _, _, w, h in regions)
        # every animation has frames of its own, all in one buffer: a third of the pixels transparent, a third opaque
        d_px = torch.randint(0, 256, (n_anim * region_bytes // 4, 4), dtype=torch.uint8, device="cuda", generator=gen)
        kind = torch.randint(0, 3, (d_px.shape[0],), device="cuda", generator=gen)
        d_px[:, 3] = torch.where(kind == 0, torch.zeros_like(d_px[:, 3]), torch.where(kind == 1, torch.full_like(d_px[:, 3], 255), d_px[:, 3]))
        del kind
        offs, at = [], 0
        for _, _, w, h in regions:
            offs.append(at)
            at += w * h * 4
        ptrs = [[d_px.data_ptr() + i * region_bytes + o for o in offs] for i in range(n_anim)]
        d_out = torch.empty(n_anim * n_fr * canvas, dtype=torch.uint8, device="cuda")
        outs = [d_out.data_ptr() + i * n_fr * canvas for i in range(n_anim)]

        def frames_of(mixed):
            return [dict(x=x, y=y, width=w, height=h, dispose_op=PAIRS[k % 6][0] if mixed else 0, blend_op=PAIRS[k % 6][1] if mixed else 0)
                    for k, (x, y, w, h) in enumerate(regions)]

        def km(mixed):
            png_compose_batch_device(eng, ptrs, [frames_of(mixed)] * n_anim, [side] * n_anim, [side] * n_anim, outs, format=PNG_RGBA8)
            return eng.stage_ms()["png_compose"]

        # KX on as many images of the canvas size: RGBA at 8 bits in, RGBA8 out
        n_img = n_anim * n_fr
        d_raw = torch.randint(0, 256, (n_img * canvas,), dtype=torch.uint8, device="cuda", generator=gen)

        def kx():
            png_expand_batch_device(eng, [d_raw.data_ptr() + i * canvas for i in range(n_img)], [side] * n_img, [side] * n_img, [8] * n_img, [6] * n_img,
                                    [d_out.data_ptr() + i * canvas for i in range(n_img)], format=PNG_RGBA8)
            return eng.stage_ms()["png_expand"]

        torch.cuda.synchronize()
        eng.set_profiling(True)
        km(False), km(True), kx()
        t = {"source": [], "mixed": [], "kx": []}
        for _ in range(a.runs):
            t["source"].append(km(False)), t["mixed"].append(km(True)), t["kx"].append(kx())
        eng.set_profiling(False)
        m = {k: statistics.median(v) for k, v in t.items()}
        km_bytes = n_anim * (n_fr * canvas + region_bytes)
        kx_bytes = 2 * n_img * canvas
        emit({"leg": "compose", "case": name, "animations": n_anim, "side": side, "frames": n_fr, "canvas_bytes_written": n_anim * n_fr * canvas,
              "region_bytes_read": n_anim * region_bytes, "km source/none (device events)": stats(t["source"]), "km six pairs in turn (device events)": stats(t["mixed"]),
              "kx on frames x animations images of the canvas size (device events)": stats(t["kx"]),
              "km source GBps written+read": round(km_bytes / m["source"] / 1e6, 1), "km mixed GBps written+read": round(km_bytes / m["mixed"] / 1e6, 1),
              "kx GBps read+written": round(kx_bytes / m["kx"] / 1e6, 1), "km source rate over kx rate": round((km_bytes / m["source"]) / (kx_bytes / m["kx"]), 3),
              "km mixed rate over kx rate": round((km_bytes / m["mixed"]) / (kx_bytes / m["kx"]), 3)})

        # ------------------------------------------------------------ whole files
        sizes = sorted({(w, h) for _, _, w, h in regions})
        stream = {}
        for w, h in sizes:
            rows = (np.add.outer(np.arange(h) * 3, np.arange(w * 4)) % 253 + np.random.default_rng(w).integers(0, 4, (h, w * 4))).astype(np.uint8)
            stream[w, h] = zlib.compress(np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes(), 1)
        f = build_file(side, side, frames_of(True), [stream[w, h] for _, _, w, h in regions])
        files = [f] * n_anim
        caps = [n_fr * canvas] * n_anim

        def whole():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st, _ = png_decode_anim_batch(eng, files, outs, caps, format=PNG_RGBA8)
            ms = (time.perf_counter() - t0) * 1e3  # (the call returns after its own wait for the stream)
            assert st == [0] * n_anim, eng.last_error()
            return ms

        whole()
        tw = [whole() for _ in range(a.runs)]
        eng.set_profiling(True)
        whole()
        stages = {k: round(v, 4) for k, v in eng.stage_ms().items() if v > 0}
        eng.set_profiling(False)
        emit({"leg": "files", "case": name, "animations": n_anim, "side": side, "frames": n_fr, "file_bytes": n_anim * len(f), "canvas_bytes_written": n_anim * n_fr * canvas,
              "zs_png_decode_anim_batch (wall clock)": stats(tw), "stages of one profiled call, ms": stages})
        del d_px, d_out, d_raw
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
