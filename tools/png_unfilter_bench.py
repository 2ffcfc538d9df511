"""PNG scanline reconstruction on the device (zs_png.hip, KU) beside the stages around it, everything resident in HBM.

Per case, in one process: the unfilter call, zs_png_filter_device on the same image (the fully parallel forward direction),
zs_inflate_batch_device on the level-6 stream of the same payload (the stage that feeds the unfilter), a device-to-device copy
of the same bytes, and the `png_segments` counter.  hipEvents on one stream, a warm-up, then the median of --reps repetitions.
Every case runs in a child process of its own, and inside it every step (set-up, check, and each of the four timings) under a
time limit of its own: a watchdog ends the process when a step overruns, the figures of the steps before it are already
printed and are kept.  The first case that fails ends the run -- nothing more is started on a device that has just failed.

    python tools/png_unfilter_bench.py [--reps 20] [--out profiles/png_unfilter.log]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("paeth3500", "sparse3500", "gradient3500", "batch256x512", "gray4096")
CASE_SECONDS = 300   # the parent's limit for a whole case; the steps inside have their own
SETUP_SECONDS = 120  # data, forward filter, level-6 deflate (and the first import of torch on a fresh machine)
STEP_SECONDS = 30    # one timing: warm-up + reps calls of a few milliseconds each


class step_limit:
    """`with step_limit(seconds, case, step):` -- the process ends (status 124, a line saying which step) if the body is still
    running after `seconds`, also when it hangs inside a device call."""

    def __init__(self, seconds, case, step):
        import threading
        self.timer = threading.Timer(seconds, self.expire)
        self.timer.daemon = True
        self.seconds, self.case, self.step = seconds, case, step

    def expire(self):
        print(json.dumps({"case": self.case, "step": self.step, "failed": "time limit of %d s" % self.seconds}), flush=True)
        os._exit(124)

    def __enter__(self):
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


def noisy_gradient(row_bytes, height, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    grad = (np.add.outer(np.arange(height) * 3, np.arange(row_bytes)) % 253).astype(np.uint8)
    return (grad + rng.integers(0, 4, grad.shape, dtype=np.uint8)).astype(np.uint8).tobytes()


def images_of(case):
    """-> (list of (pixels, row_bytes, height, bpp), forward filter type)"""
    from zlibstream_amd import datagen
    if case == "paeth3500":
        return [(noisy_gradient(3500 * 4, 3500, 1), 3500 * 4, 3500, 4)], 4
    if case == "sparse3500":
        return [(datagen.sparse(3500, 3500), 3500 * 4, 3500, 4)], 5
    if case == "gradient3500":
        return [(noisy_gradient(3500 * 4, 3500, 2), 3500 * 4, 3500, 4)], 5
    if case == "batch256x512":
        return [(noisy_gradient(512 * 4, 512, 100 + i) if i % 2 else datagen.sparse(512, 512), 512 * 4, 512, 4) for i in range(256)], 5
    if case == "gray4096":
        return [(noisy_gradient(4096, 4096, 3), 4096, 4096, 1)], 5
    raise SystemExit("unknown case " + case)


def median_ms(fn, stream, reps):
    import torch
    fn()
    fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def run_case(case, reps):
    import torch
    from zlibstream_amd import Engine, deflate_bound, png_filter_device, png_unfilter_batch_device
    with step_limit(SETUP_SECONDS, case, "setup"):
        eng = Engine(0)
        images, ftype = images_of(case)
        n = len(images)
        stream = torch.cuda.Stream()
        sp = stream.cuda_stream
        d_img = [torch.frombuffer(bytearray(p), dtype=torch.uint8).cuda() for p, _, _, _ in images]
        d_f = [torch.zeros(h * (rb + 1), dtype=torch.uint8, device="cuda") for _, rb, h, _ in images]
        d_back = [torch.zeros(h * rb, dtype=torch.uint8, device="cuda") for _, rb, h, _ in images]
        rbs, hs, bpps = [rb for _, rb, _, _ in images], [h for _, _, h, _ in images], [b for _, _, _, b in images]
        pixels = sum(rb * h for rb, h in zip(rbs, hs))
        torch.cuda.synchronize()

        def forward():
            for i in range(n):
                png_filter_device(eng, d_img[i].data_ptr(), rbs[i], hs[i], bpps[i], ftype, d_f[i].data_ptr(), stream=sp)

        with torch.cuda.stream(stream):
            forward()
            stream.synchronize()
            f_len = [t.numel() for t in d_f]
            caps = [deflate_bound(x) for x in f_len]
            d_z = [torch.empty(c, dtype=torch.uint8, device="cuda") for c in caps]
            z_len = eng.deflate_batch_device([t.data_ptr() for t in d_f], f_len, [t.data_ptr() for t in d_z], caps, level=6, stream=sp)
            d_idat = [torch.zeros(x, dtype=torch.uint8, device="cuda") for x in f_len]

    def inflate():
        eng.inflate_batch_device([t.data_ptr() for t in d_z], z_len, [t.data_ptr() for t in d_idat], f_len, stream=sp)

    def unfilter():
        st = png_unfilter_batch_device(eng, [t.data_ptr() for t in d_idat], rbs, hs, bpps, [t.data_ptr() for t in d_back], stream=sp)
        assert not any(st), st

    def copy():
        for i in range(n):
            d_back[i].copy_(d_img[i], non_blocking=True)

    row = {"case": case, "images": n, "pixel_bytes": pixels, "compressed_bytes": int(sum(z_len)), "reps": reps}
    with torch.cuda.stream(stream):
        with step_limit(STEP_SECONDS, case, "check"):
            inflate()
            unfilter()
            row["png_segments"] = eng.counter("png_segments")
            exact = all(torch.equal(a, b) for a, b in zip(d_back, d_img))
            row["inflate->unfilter gives the pixels back"] = exact
        ms = {}
        for step, fn in (("unfilter", unfilter), ("filter", forward), ("inflate", inflate), ("copy", copy)):
            with step_limit(STEP_SECONDS, case, step):
                ms[step] = median_ms(fn, stream, reps)
            row[step + "_ms"] = round(ms[step], 4)
            row[step + "_GBps"] = round(pixels / ms[step] / 1e6, 2)
            print(json.dumps({"case": case, "step": step, "ms": row[step + "_ms"], "GBps": row[step + "_GBps"]}), flush=True)
    row["unfilter_over_inflate"] = round(ms["unfilter"] / ms["inflate"], 3)
    print(json.dumps(row), flush=True)
    return 0 if exact else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_unfilter.log"))
    a = ap.parse_args()
    if a.case:
        sys.exit(run_case(a.case, a.reps))
    lines = []
    for case in CASES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)], capture_output=True, text=True,
                               timeout=CASE_SECONDS)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps({"case": case, "failed": "time limit of %d s" % CASE_SECONDS}))
            break
        out = [x for x in r.stdout.splitlines() if x.startswith("{")]
        rows = [x for x in out if '"step"' not in x]
        lines += rows if r.returncode == 0 and rows else out  # (a case that failed keeps the figures of the steps it finished)
        if r.returncode != 0 or not rows:
            lines.append(json.dumps({"case": case, "failed": "exit %d" % r.returncode, "stderr": r.stderr[-500:]}))
            break  # nothing more is started on a device that has just failed
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(0 if len(lines) == len(CASES) and not any('"failed"' in x for x in lines) else 1)


if __name__ == "__main__":
    main()
