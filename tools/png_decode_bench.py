"""The PNG decode call (zs_png_decode_batch_device) and the Adam7 interleave kernel (zs_png.hip, KA), everything resident in HBM.

KA cases: zs_png_adam7_merge_batch_device on random pass bytes beside a device-to-device copy of as many bytes -- the yardstick:
KA reads and writes every byte once, as a copy does -- with the group width of a lane (ZS_PNG_A7_GROUP = 4, 8, 16 bytes; the
library's default without it).  hipEvents on one stream, a warm-up, then the median of --reps repetitions; the events span
the call's descriptor upload and its wait for it too, so tools/prof_one.sh-style kernel traces give the kernel alone.
Fused cases: the decode call against the caller's way with the entry points that were there before it -- inflate_batch_device,
png_unfilter_batch_device (seven entries per interlaced image), and for interlaced images a copy to the host, a numpy
interleave and a copy back.  Wall-clock medians of --reps calls, each ended by a device synchronisation.
Every case runs in a child process of its own and every step under a time limit; the first case that fails ends the run.

    python tools/png_decode_bench.py [--reps 20] [--out profiles/png_decode_batch.log]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.png_unfilter_bench import median_ms, noisy_gradient, step_limit  # noqa: E402

KA_SHAPES = {"ka1x4096": (1, 4096, 4096), "ka256x512": (256, 512, 512)}
CASES = [(shape + "_%dbit" % bits, group) for shape in KA_SHAPES for bits in (32, 1) for group in (4, 8, 16)] + \
    [("fused_interlaced256x512", 0), ("fused_batch256x512", 0)]
CASE_SECONDS, SETUP_SECONDS, STEP_SECONDS = 300, 150, 60
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))  # PNG specification 8.2


def interleave_numpy(blob, w, h, bits):
    """the passes of one image back to back (no filter bytes) -> its raw scanlines, by the table"""
    import numpy as np
    px = np.zeros((h, w) if bits < 8 else (h, w, bits // 8), dtype=np.uint8)
    at = 0
    for xs, ys, xst, yst in ADAM7:
        pw, ph = len(range(xs, w, xst)), len(range(ys, h, yst))
        if not pw or not ph:
            continue
        rb = (pw * bits + 7) // 8
        rows = blob[at:at + rb * ph].reshape(ph, rb)
        at += rb * ph
        px[ys::yst, xs::xst] = rows.reshape(ph, pw, bits // 8) if bits >= 8 else np.unpackbits(rows, axis=1)[:, :pw]
    return px.reshape(h, -1) if bits >= 8 else np.packbits(px, axis=1)


def run_ka(case, reps):
    import numpy as np
    import torch
    from zlibstream_amd import Engine, png_adam7_merge_batch_device, png_idat_layout
    shape, bits = case.split("_")
    n, w, h = KA_SHAPES[shape]
    bits = int(bits[:-3])
    with step_limit(SETUP_SECONDS, case, "setup"):
        eng = Engine(0)
        stream = torch.cuda.Stream()
        _, rb7, rows7 = png_idat_layout(w, h, bits, 1)
        n_in, n_out = sum(b * r for b, r in zip(rb7, rows7)), h * ((w * bits + 7) // 8)
        d_in = [torch.randint(0, 256, (n_in,), dtype=torch.uint8, device="cuda") for _ in range(n)]
        d_out = [torch.zeros(n_out, dtype=torch.uint8, device="cuda") for _ in range(n)]
        d_copy = [torch.zeros(n_out, dtype=torch.uint8, device="cuda") for _ in range(n)]
        args = ([t.data_ptr() for t in d_in], [w] * n, [h] * n, [bits] * n, [t.data_ptr() for t in d_out])
        torch.cuda.synchronize()

    def merge():
        png_adam7_merge_batch_device(eng, *args, stream=stream.cuda_stream)

    def copy():
        for i in range(n):
            d_copy[i].copy_(d_in[i][:n_out], non_blocking=True)

    row = {"case": case, "group": os.environ.get("ZS_PNG_A7_GROUP", "default"), "images": n, "bits": bits, "out_bytes": n * n_out, "reps": reps}
    with torch.cuda.stream(stream):
        with step_limit(STEP_SECONDS, case, "check"):
            merge()
            stream.synchronize()
            exact = interleave_numpy(d_in[n - 1].cpu().numpy(), w, h, bits).tobytes() == d_out[n - 1].cpu().numpy().tobytes()
            row["merge is the table's interleave"] = exact
        for step, fn in (("merge", merge), ("copy", copy)):
            with step_limit(STEP_SECONDS, case, step):
                ms = median_ms(fn, stream, reps)
            row[step + "_ms"], row[step + "_GBps"] = round(ms, 4), round(n * n_out / ms / 1e6, 2)
    row["merge_over_copy"] = round(row["merge_ms"] / row["copy_ms"], 2)
    print(json.dumps(row), flush=True)
    return 0 if exact else 1


def wall_ms(fn, reps):
    import torch
    fn()
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def run_fused(case, reps):
    import numpy as np
    import torch
    from zlibstream_amd import (Engine, datagen, deflate_bound, png_decode_batch_device, png_filter_batch_device, png_idat_layout,
                                png_unfilter_batch_device)
    interlace = 1 if "interlaced" in case else 0
    n, w, h, bits = 256, 512, 512, 32
    with step_limit(SETUP_SECONDS, case, "setup"):
        eng = Engine(0)
        imgs = [np.frombuffer(noisy_gradient(w * 4, h, 100 + i) if i % 2 else datagen.sparse(w, h), dtype=np.uint8).reshape(h, w, 4) for i in range(n)]
        need, rb7, rows7 = png_idat_layout(w, h, bits, interlace)
        parts = [(rb, rows) for rb, rows in zip(rb7, rows7) if rows]
        # the passes as images of their own (or the image), filtered on the device into the IDAT payload, deflated at level 6
        if interlace:
            host = [np.concatenate([im[ys::yst, xs::xst].reshape(-1) for xs, ys, xst, yst in ADAM7]) for im in imgs]
        else:
            host = [im.reshape(-1) for im in imgs]
        d_px = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in host]
        d_payload = [torch.zeros(need, dtype=torch.uint8, device="cuda") for _ in range(n)]
        src, dst, rbs, hs = [], [], [], []
        for i in range(n):
            a = b = 0
            for rb, rows in parts:
                src.append(d_px[i].data_ptr() + a), dst.append(d_payload[i].data_ptr() + b), rbs.append(rb), hs.append(rows)
                a, b = a + rb * rows, b + (rb + 1) * rows
        torch.cuda.synchronize()
        png_filter_batch_device(eng, src, rbs, hs, [4] * len(src), [5] * len(src), dst)
        cap = deflate_bound(need)
        d_z = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        z_len = eng.deflate_batch_device([t.data_ptr() for t in d_payload], [need] * n, [t.data_ptr() for t in d_z], [cap] * n, level=6)
        d_out = [torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(n)]
        d_mid = [torch.zeros(need, dtype=torch.uint8, device="cuda") for _ in range(n)]
        d_passes = [torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(n)]
        d_way = [torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(n)]
        z_ptrs, out_ptrs = [t.data_ptr() for t in d_z], [t.data_ptr() for t in d_out]
        torch.cuda.synchronize()

    def fused():
        st = png_decode_batch_device(eng, z_ptrs, z_len, [w] * n, [h] * n, [bits] * n, [interlace] * n, out_ptrs)
        assert not any(st), st

    def callers_way():
        eng.inflate_batch_device(z_ptrs, z_len, [t.data_ptr() for t in d_mid], [need] * n)
        u_in, u_out = [], []
        for i in range(n):
            a = b = 0
            for rb, rows in parts:
                u_in.append(d_mid[i].data_ptr() + b), u_out.append((d_passes if interlace else d_way)[i].data_ptr() + a)
                a, b = a + rb * rows, b + (rb + 1) * rows
        st = png_unfilter_batch_device(eng, u_in, rbs, hs, [4] * len(u_in), u_out)
        assert not any(st), st
        if interlace:
            for i in range(n):
                d_way[i].copy_(torch.from_numpy(interleave_numpy(d_passes[i].cpu().numpy(), w, h, bits).reshape(-1)))

    row = {"case": case, "images": n, "pixel_bytes": n * w * h * 4, "compressed_bytes": int(sum(z_len)), "reps": reps}
    with step_limit(STEP_SECONDS, case, "check"):
        fused()
        callers_way()
        torch.cuda.synchronize()
        exact = all(torch.equal(a, torch.from_numpy(im.reshape(-1)).cuda()) and torch.equal(a, b) for a, b, im in zip(d_out, d_way, imgs))
        row["both ways give the pixels back"] = exact
    for step, fn, k in (("decode_call", fused, reps), ("callers_way", callers_way, reps if not interlace else max(3, reps // 5))):
        with step_limit(2 * STEP_SECONDS, case, step):
            row[step + "_ms"] = round(wall_ms(fn, k), 3)
    row["decode_call_over_callers_way"] = round(row["decode_call_ms"] / row["callers_way_ms"], 3)
    print(json.dumps(row), flush=True)
    return 0 if exact else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode_batch.log"))
    a = ap.parse_args()
    if a.case:
        sys.exit((run_ka if a.case.startswith("ka") else run_fused)(a.case, a.reps))
    lines, failed = [], False
    for case, group in CASES:
        env = dict(os.environ)
        env.pop("ZS_PNG_A7_GROUP", None)
        if group:
            env["ZS_PNG_A7_GROUP"] = str(group)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)], capture_output=True, text=True,
                               timeout=CASE_SECONDS, env=env)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps({"case": case, "failed": "time limit of %d s" % CASE_SECONDS}))
            failed = True
            break
        rows = [x for x in r.stdout.splitlines() if x.startswith("{")]
        lines += rows
        if r.returncode != 0 or not rows:
            lines.append(json.dumps({"case": case, "failed": "exit %d" % r.returncode, "stderr": r.stderr[-500:]}))
            failed = True
            break  # nothing more is started on a device that has just failed
        print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
