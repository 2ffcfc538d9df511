"""Animated PNG on the way out: the frame diff (zs_png_diff_batch_device, KD) and the crop beside a device-to-device copy of
the bytes each reads, and a whole zs_png_encode_anim_batch_device call beside the only way there was before it, the same
canvases as frames x animations still images through zs_png_encode_rgba_batch_device.

    kernels       KD over the canvases and the crop over the regions KD found, by device events (zs_ctx_stage_ms "png_diff",
                  "png_crop"); the copy of as many bytes (torch's copy_ between two device buffers) by device events too.  KD
                  reads every canvas once and writes next to nothing, the copy reads and writes, so "rate over copy" compares
                  bytes read per second.
    files         wall-clock milliseconds around each call (both end in their own wait for the stream), the files' total bytes,
                  and the stages of one profiled call with the share of png_diff + png_crop in it.

The cases are those of profiles/png_anim.log: one 1024 x 1024 animation of 64 frames in which every pixel changes; one in
which a 64 x 64 cell changes per frame; 256 animations of 128 x 128 with 16 frames in which every pixel changes.  Every leg
is warmed up once, then the legs alternate --runs times: median and spread (max - min).

    python tools/png_anim_encode_bench.py [--runs 7] [--level 6] [--out profiles/png_anim_encode.log]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--scale", type=int, default=1, help="divide the canvases' sides by this (a rehearsal; 1 for the log)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_anim_encode.log"))
    a = ap.parse_args()
    import torch
    from zlibstream_amd import (Engine, PNG_RGBA8, deflate_bound, png_anim_bound, png_crop_batch_device, png_diff_batch_device, png_encode_anim_batch_device,
                                png_encode_rgba_batch_device, png_file_bound, png_idat_layout)
    if not torch.cuda.is_available():
        sys.exit("png_anim_encode_bench: no GPU (there is nothing to measure without one)")
    eng = Engine(0)
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}

    def copy_ms(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def run():
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run

    big, small, cell = 1024 // a.scale, 128 // a.scale, 64 // a.scale
    cases = (("1 animation, 64 frames, every pixel changes", 1, big, 64, 0), ("1 animation, 64 frames, a cell of a 16th of the side changes", 1, big, 64, cell),
             ("256 animations, 16 frames, every pixel changes", 256, small, 16, 0))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    for name, n_anim, side, n_fr, cell_side in cases:
        canvas = side * side * 4
        # a noisy gradient (it deflates, but not to nothing); every pixel changes: the picture moves; a cell changes: a cell of new noise
        yy, xx = torch.meshgrid(torch.arange(side, device="cuda"), torch.arange(side, device="cuda"), indexing="ij")
        base = torch.stack([(xx * 3 + yy) % 253, (xx + yy * 2) % 251, (xx * 2 + yy * 5) % 241, torch.full_like(xx, 255)], dim=2)
        d_cv = torch.empty((n_anim, n_fr, side, side, 4), dtype=torch.uint8, device="cuda")
        for i in range(n_anim):
            cur = ((base + torch.randint(0, 4, base.shape, device="cuda", generator=gen)) % 256).to(torch.uint8)
            cur[..., 3] = 255
            for f in range(n_fr):
                if f and cell_side:
                    g = side // cell_side
                    x, y = (f % g) * cell_side, (f * 5 % g) * cell_side
                    cur = cur.clone()
                    cur[y:y + cell_side, x:x + cell_side, :3] += torch.randint(1, 8, (cell_side, cell_side, 3), dtype=torch.uint8, device="cuda", generator=gen)
                elif f:
                    cur = torch.roll(cur, (1, 3), dims=(0, 1))
                    cur[..., 0] += 1
                d_cv[i, f] = cur
        ptrs = [d_cv[i].data_ptr() for i in range(n_anim)]
        nf, sides = [n_fr] * n_anim, [side] * n_anim
        torch.cuda.synchronize()
        regions = png_diff_batch_device(eng, ptrs, nf, sides, sides, format=PNG_RGBA8)
        # ------------------------------------------------------------ the two kernels beside a copy
        crop_in, crop_iw, crop_x, crop_y, crop_w, crop_h = [], [], [], [], [], []
        for i in range(n_anim):
            for f in range(1, n_fr):
                r = regions[i][f]
                crop_in.append(d_cv[i, f].data_ptr()), crop_iw.append(side), crop_x.append(r["x"]), crop_y.append(r["y"]), crop_w.append(r["width"]), crop_h.append(r["height"])
        crop_bytes = sum(w * h * 4 for w, h in zip(crop_w, crop_h))
        d_crop = torch.empty(crop_bytes + 256 * len(crop_w), dtype=torch.uint8, device="cuda")
        crop_out, at = [], 0
        for w, h in zip(crop_w, crop_h):
            crop_out.append(d_crop.data_ptr() + at)
            at += (w * h * 4 + 255) // 256 * 256

        def kd():
            png_diff_batch_device(eng, ptrs, nf, sides, sides, format=PNG_RGBA8)
            return eng.stage_ms()["png_diff"]

        def crop():
            png_crop_batch_device(eng, crop_in, crop_iw, crop_x, crop_y, crop_w, crop_h, crop_out, pixel_bytes=4)
            return eng.stage_ms()["png_crop"]

        diff_bytes = n_anim * n_fr * canvas
        copy_all, copy_regions = copy_ms(diff_bytes), copy_ms(max(crop_bytes, 1))
        eng.set_profiling(True)
        kd(), crop(), copy_all(), copy_regions()
        t = {"kd": [], "crop": [], "copy_all": [], "copy_regions": []}
        for _ in range(a.runs):
            t["kd"].append(kd()), t["copy_all"].append(copy_all()), t["crop"].append(crop()), t["copy_regions"].append(copy_regions())
        eng.set_profiling(False)
        m = {k: statistics.median(v) for k, v in t.items()}
        emit({"leg": "kernels", "case": name, "animations": n_anim, "side": side, "frames": n_fr, "canvas_bytes_read_by_kd": diff_bytes, "region_bytes_read_by_the_crop": crop_bytes,
              "kd, both launches (device events)": stats(t["kd"]), "copy of the canvases' bytes (device events)": stats(t["copy_all"]),
              "crop of every later frame's region (device events)": stats(t["crop"]), "copy of the regions' bytes (device events)": stats(t["copy_regions"]),
              "kd GBps read": round(diff_bytes / m["kd"] / 1e6, 1), "copy GBps read": round(diff_bytes / m["copy_all"] / 1e6, 1),
              "kd rate over copy rate": round(m["copy_all"] / m["kd"], 3), "crop GBps read": round(crop_bytes / m["crop"] / 1e6, 1),
              "crop rate over copy rate": round(m["copy_regions"] / m["crop"], 3)})
        del d_crop
        # ------------------------------------------------------------ whole calls
        cap_anim = png_anim_bound(side, side, n_fr, PNG_RGBA8, 0, 0, 0)
        cap_still = png_file_bound(deflate_bound(png_idat_layout(side, side, 32, 0)[0]), 0, 1048)
        d_out = torch.empty(max(n_anim * cap_anim, n_anim * n_fr * cap_still), dtype=torch.uint8, device="cuda")
        anim_out = [d_out.data_ptr() + i * cap_anim for i in range(n_anim)]
        still_px = [d_cv[i, f].data_ptr() for i in range(n_anim) for f in range(n_fr)]
        still_out = [d_out.data_ptr() + k * cap_still for k in range(n_anim * n_fr)]
        got = {}

        def anim():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lens = png_encode_anim_batch_device(eng, ptrs, nf, sides, sides, [5] * n_anim, anim_out, [cap_anim] * n_anim, format=PNG_RGBA8, level=a.level)[0]
            ms = (time.perf_counter() - t0) * 1e3  # (the call returns after its own wait for the stream)
            got["anim"] = sum(lens)
            return ms

        def stills():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lens = png_encode_rgba_batch_device(eng, still_px, [side] * len(still_px), [side] * len(still_px), [5] * len(still_px), still_out,
                                                [cap_still] * len(still_px), format=PNG_RGBA8, level=a.level)[0]
            ms = (time.perf_counter() - t0) * 1e3
            got["stills"] = sum(lens)
            return ms

        anim(), stills()
        ta, ts = [], []
        for _ in range(a.runs):
            ta.append(anim()), ts.append(stills())
        eng.set_profiling(True)
        anim()
        stages = {k: round(v, 4) for k, v in eng.stage_ms().items() if v > 0}
        eng.set_profiling(False)
        front = stages.get("png_diff", 0) + stages.get("png_crop", 0)
        emit({"leg": "files", "case": name, "animations": n_anim, "side": side, "frames": n_fr, "level": a.level, "filter": 5, "canvas_bytes": diff_bytes,
              "zs_png_encode_anim_batch_device (wall clock)": stats(ta), "zs_png_encode_rgba_batch_device on frames x animations stills (wall clock)": stats(ts),
              "animated file bytes": got["anim"], "still files' bytes": got["stills"], "animated over stills, time": round(statistics.median(ta) / statistics.median(ts), 3),
              "animated over stills, bytes": round(got["anim"] / got["stills"], 4), "stages of one profiled animated call, ms": stages,
              "png_diff + png_crop, ms": round(front, 4), "their share of the stages' sum": round(front / max(sum(stages.values()), 1e-9), 4),
              "their share of the call's wall clock": round(front / statistics.median(ta), 4)})
        del d_cv, d_out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
