"""The PNG encoder direction on the device, a batch of images a call against one image a call, everything resident in HBM.

Two libraries alternate in one job, --runs times each (a child process per run, so that neither sees the other's warm buffers):
the parent commit's build (--parent-lib, which has only the one-image entries) and this tree's.  Per case and level a run times

    loop_filter    n calls of zs_png_filter_device on the caller's stream, one wait at the end   (n launches of the old kernel)
    loop_deflate   n calls of zs_deflate_writes_device, one Write per row (and the longest of the n calls on its own)
    batch_filter   zs_png_filter_batch_device                                                    (one launch of the new kernel)
    batch_deflate  zs_deflate_writes_batch_device on the same rows and Write lists
    idat           zs_png_idat_batch_device: the two in one call

(the batch legs on this tree's library only), checks that the batch's streams are the loop's byte for byte, and reports the
stage times of one profiled batch_deflate call.  batch_filter_unstaged is the batch filter kernel with ZS_PNG_NO_STAGE=1, its rows
read from memory as the one-image kernel reads them.  Wall-clock milliseconds around each leg, the device idle before and after.
A last row per run of this tree's library, periodic_beside_list, is what a list costs its neighbours at level 1: 1 MiB of zeros
as one Write alone (planned for the speculative runs' engine), in a batch beside a 4 KiB stream with a Write list, and in a plain
zs_deflate_batch_device call beside the same 4 KiB without a list (the sweeps both times: the runs' engine is for batches whose
streams are all of 256 KiB .. 4 MiB and all one Write).

Cases: 256 x (512 x 512 RGBA, sparse and noisy gradients in turn) and 16 x (3500 x 3500 RGBA datagen.sparse), adaptive filter,
levels 1 and 6.  At level 1 one Write per row puts these streams on the one-wave literal engine (zs_core.h build_read_events
takes neither schedule), about a second per MiB and stream: level 1 is timed on the first --l1-images images of the first case
(8: 8 s a loop) and not at all on the second (49 MB a stream) unless --l1-big is given.

    python tools/png_encode_bench.py --parent-lib build/libzsgpu_parent.so [--runs 5] [--out profiles/png_encode_batch.log]
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

CASES = ("batch256x512", "sparse16x3500")
RUN_SECONDS = 420  # the parent's limit for one child: set-up, and every leg of both cases at both levels
LEGS = ("loop_filter", "loop_deflate", "batch_filter_unstaged", "batch_filter", "batch_deflate", "idat")


def noisy_gradient(row_bytes, height, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    grad = (np.add.outer(np.arange(height) * 3, np.arange(row_bytes)) % 253).astype(np.uint8)
    return (grad + rng.integers(0, 4, grad.shape, dtype=np.uint8)).astype(np.uint8).tobytes()


def images_of(case):
    from zlibstream_amd import datagen
    if case == "batch256x512":
        return [(noisy_gradient(2048, 512, 100 + i) if i % 2 else datagen.sparse(512, 512, y0=i), 2048, 512, 4) for i in range(256)]
    one = datagen.sparse(3500, 3500)
    return [(one, 14000, 3500, 4)] * 16  # (the same pixels in 16 device buffers of their own)


def run_child(a):
    """One run of one library: every case and level, a JSON line per (case, level)."""
    import ctypes
    import threading
    import torch
    from zlibstream_amd import Engine, _native, deflate_bound, png_filter_device
    threading.Timer(RUN_SECONDS - 10, lambda: (print(json.dumps({"failed": "time limit"}), flush=True), os._exit(124))).start()
    has_batch = hasattr(_native.lib(), "zs_png_filter_batch_device")
    if has_batch:
        from zlibstream_amd import png_filter_batch_device, png_idat_batch_device
    eng = Engine(0)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for case in CASES:
        images = images_of(case)
        for level in (6, 1):
            if level == 1 and case != CASES[0] and not a.l1_big:
                continue
            imgs = images[:a.l1_images] if level == 1 and case == CASES[0] else images
            n = len(imgs)
            rbs, hs, bpps = [x[1] for x in imgs], [x[2] for x in imgs], [x[3] for x in imgs]
            flen = [h * (rb + 1) for rb, h in zip(rbs, hs)]
            caps = [deflate_bound(x) + 64 * h for x, h in zip(flen, hs)]
            d_img = [torch.frombuffer(bytearray(x[0]), dtype=torch.uint8).cuda() for x in imgs]
            d_f = [torch.zeros(x, dtype=torch.uint8, device="cuda") for x in flen]
            d_fb = [torch.zeros(x, dtype=torch.uint8, device="cuda") for x in flen]
            d_z = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
            d_zb = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
            ends = [(ctypes.c_int64 * h)(*[(r + 1) * (rb + 1) for r in range(h)]) for rb, h in zip(rbs, hs)]
            torch.cuda.synchronize()
            lens, blens, each = [0] * n, [0] * n, [0.0] * n

            def loop_filter():
                for i in range(n):
                    png_filter_device(eng, d_img[i].data_ptr(), rbs[i], hs[i], bpps[i], 5, d_f[i].data_ptr(), stream=sp)

            def loop_deflate():
                for i in range(n):
                    t0 = time.perf_counter()
                    lens[i] = eng.deflate_writes_device(d_f[i].data_ptr(), flen[i], ends[i], d_z[i].data_ptr(), caps[i], level=level, stream=sp)
                    each[i] = (time.perf_counter() - t0) * 1e3  # (the call has waited for the stream: it returns the length)

            def batch_filter():
                png_filter_batch_device(eng, [t.data_ptr() for t in d_img], rbs, hs, bpps, [5] * n, [t.data_ptr() for t in d_fb], stream=sp)

            def batch_filter_unstaged():
                os.environ["ZS_PNG_NO_STAGE"] = "1"  # (read by the library at every call)
                try:
                    batch_filter()
                finally:
                    del os.environ["ZS_PNG_NO_STAGE"]

            def batch_deflate():
                blens[:] = eng.deflate_writes_batch_device([t.data_ptr() for t in d_fb], flen, ends, [t.data_ptr() for t in d_zb], caps, level=level, stream=sp)

            def idat():
                blens[:] = png_idat_batch_device(eng, [t.data_ptr() for t in d_img], rbs, hs, bpps, [5] * n, [t.data_ptr() for t in d_zb], caps,
                                                 rows_per_write=1, level=level, stream=sp)

            legs = [("loop_filter", loop_filter), ("loop_deflate", loop_deflate)]
            if has_batch:
                legs += [("batch_filter_unstaged", batch_filter_unstaged), ("batch_filter", batch_filter), ("batch_deflate", batch_deflate), ("idat", idat)]
            row = {"lib": a.tag, "run": a.run, "case": case, "level": level, "images": n, "pixel_bytes": sum(rb * h for rb, h in zip(rbs, hs))}
            for name, fn in legs:
                if level != 1 or "filter" in name:
                    timed(fn)  # warm-up: the workspace grows on a first call (not at level 1, where a call is seconds of one wave)
                row[name + "_ms"] = round(timed(fn), 3)
            row["loop_deflate_longest_call_ms"] = round(max(each), 3)
            if has_batch:
                row["batch is the loop byte for byte"] = bool(lens == list(blens) and all(torch.equal(x, y) for x, y in zip(d_f, d_fb)) and
                                                              all(torch.equal(x[:k], y[:k]) for x, y, k in zip(d_z, d_zb, lens)))
                if level != 1:
                    eng.set_profiling(True)
                    timed(batch_deflate)
                    row["batch_deflate_stage_ms"] = {k: round(v, 3) for k, v in eng.stage_ms().items() if v >= 0.01}
                    eng.set_profiling(False)
            row["compressed_bytes"] = int(sum(lens))
            print(json.dumps(row), flush=True)
            del d_img, d_f, d_fb, d_z, d_zb
    if has_batch:
        zeros = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
        small = torch.frombuffer(bytearray(noisy_gradient(64, 64, 7)), dtype=torch.uint8).cuda()
        outs = [torch.zeros(deflate_bound(1 << 20), dtype=torch.uint8, device="cuda") for _ in range(2)]
        ptrs, caps = [t.data_ptr() for t in outs], [t.numel() for t in outs]
        dual = {"zeros_alone": lambda: eng.deflate_batch_device([zeros.data_ptr()], [1 << 20], ptrs[:1], caps[:1], level=1, stream=sp),
                "list_alone": lambda: eng.deflate_writes_device(small.data_ptr(), 4096, [100, 4096], ptrs[1], caps[1], level=1, stream=sp),
                "zeros_beside_list": lambda: eng.deflate_writes_batch_device([zeros.data_ptr(), small.data_ptr()], [1 << 20, 4096], [None, [100, 4096]],
                                                                             ptrs, caps, level=1, stream=sp),
                "zeros_beside_plain": lambda: eng.deflate_batch_device([zeros.data_ptr(), small.data_ptr()], [1 << 20, 4096], ptrs, caps, level=1, stream=sp)}
        row = {"lib": a.tag, "run": a.run, "case": "periodic_beside_list", "level": 1}
        for name, fn in dual.items():
            timed(fn)
            row[name + "_ms"] = round(timed(fn), 3)
        print(json.dumps(row), flush=True)
    os._exit(0)


def table(rows, runs):
    """Median and spread (max - min) of every leg over the runs, per case and level, and the verdicts."""
    out = []
    for case in CASES:
        for level in (6, 1):
            sel = [r for r in rows if r.get("case") == case and r.get("level") == level]
            if not sel:
                continue
            out.append("## %s, level %d, %d images, one Write per row (ms: median of %d runs, spread = max - min)" % (case, level, sel[0]["images"], runs))
            stat = {}
            for lib in ("parent", "branch"):
                for leg in LEGS:
                    v = [r[leg + "_ms"] for r in sel if r["lib"] == lib and leg + "_ms" in r]
                    if v:
                        stat[lib, leg] = (statistics.median(v), max(v) - min(v))
                        out.append("%-15s %-14s %10.3f   spread %8.3f   runs %s" % (lib, leg, stat[lib, leg][0], stat[lib, leg][1], " ".join("%.3f" % x for x in v)))
            v = [r["loop_deflate_longest_call_ms"] for r in sel if r["lib"] == "branch"]
            if v:
                out.append("branch          longest single call of loop_deflate %10.3f" % statistics.median(v))
            for lib in ("parent", "branch"):
                v = [r["loop_filter_ms"] + r["loop_deflate_ms"] for r in sel if r["lib"] == lib]
                if v:
                    stat[lib, "loop"] = (statistics.median(v), max(v) - min(v))
            v = [r["idat_ms"] for r in sel if r["lib"] == "branch"]
            if v and ("parent", "loop") in stat:
                p, spread = stat["parent", "loop"]
                b, bl = statistics.median(v), stat["branch", "loop"][0]
                out.append("parent loop (filter + deflate) %.3f, spread %.3f | branch loop %.3f | branch batch (idat) %.3f = %.1f x" % (p, spread, bl, b, p / b))
                out.append("verdict: batch %s the parent's loop + spread; branch loop %s the parent's loop + spread" %
                           ("within" if b <= p + spread else "SLOWER THAN", "within" if bl <= p + spread else "SLOWER THAN"))
            st = [r["batch_deflate_stage_ms"] for r in sel if "batch_deflate_stage_ms" in r]
            if st:
                out.append("stages of one profiled batch_deflate call: " + json.dumps(st[len(st) // 2]))
            out.append("")
    sel = [r for r in rows if r.get("case") == "periodic_beside_list"]
    if sel:
        out.append("## level 1: 1 MiB of zeros, one Write, alone, beside a 4 KiB stream with a Write list, beside the same without one (ms: median of %d runs)" % len(sel))
        for leg in ("zeros_alone", "list_alone", "zeros_beside_list", "zeros_beside_plain"):
            v = [r[leg + "_ms"] for r in sel]
            out.append("%-18s %10.3f   spread %8.3f   runs %s" % (leg, statistics.median(v), max(v) - min(v), " ".join("%.3f" % x for x in v)))
        out.append("")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libzsgpu.so built from the parent commit")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--l1-images", type=int, default=8)
    ap.add_argument("--l1-big", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode_batch.log"))
    ap.add_argument("--tag")
    ap.add_argument("--run", type=int, default=0)
    a = ap.parse_args()
    if a.tag:
        run_child(a)
    plan = []
    for k in range(a.runs):
        if a.parent_lib:
            plan.append(("parent", k, {"ZS_DEV": "1", "ZS_LIB": os.path.abspath(a.parent_lib)}))
        plan.append(("branch", k, {}))
    rows, failed = [], None
    for tag, k, env in plan:
        cmd = [sys.executable, os.path.abspath(__file__), "--tag", tag, "--run", str(k), "--l1-images", str(a.l1_images)] + (["--l1-big"] if a.l1_big else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=RUN_SECONDS, env=dict(os.environ, **env))
        except subprocess.TimeoutExpired:
            failed = "%s run %d: time limit of %d s" % (tag, k, RUN_SECONDS)
            break
        got = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
        rows += got
        for x in got:
            print(json.dumps(x), flush=True)
        if r.returncode != 0 or not got or any("failed" in x or x.get("batch is the loop byte for byte") is False for x in got):
            failed = "%s run %d: exit %d: %s" % (tag, k, r.returncode, r.stderr[-500:])
            break  # nothing more is started on a device that has just failed
    lines = [json.dumps(x) for x in rows] + [""] + table(rows, a.runs)
    if failed:
        lines.append("FAILED: " + failed)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[len(rows):]))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
