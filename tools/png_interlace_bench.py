"""The Adam7 split kernel (zs_png.hip, KS) and the interlaced encode call (zs_png_encode_interlace_batch_device), everything
resident in HBM.

KS cases: zs_png_adam7_split_batch_device on random pixels, timed by the context's stage timer ("png_split": the launches alone,
between two events) beside a device-to-device copy of as many bytes -- the yardstick: KS writes every byte once and reads about
as many, as a copy does -- with the group width of a lane (ZS_PNG_SPLIT_GROUP = 4, 8, 16 bytes; the library's default without
it).  A warm-up, then the median of --reps repetitions.
Encode cases: the whole call at level 6 with interlace 1 against interlace 0 on the same pixels, with one Write per row (pass
rows for interlace 1) and with one Write per image.  Interlaced streams compress worse, have about 1.9 x the Writes, and their
first passes' rows are an eighth of a row long: a ratio to record, not one to assert.  Wall-clock medians of --reps calls, each
ended by a device synchronisation.
Every case runs in a child process of its own and every step under a time limit; the first case that fails ends the run.

    python tools/png_interlace_bench.py [--reps 20] [--out profiles/png_interlace.log]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.png_decode_bench import wall_ms  # noqa: E402
from tools.png_unfilter_bench import median_ms, noisy_gradient, step_limit  # noqa: E402

SHAPES = {"1x4096": (1, 4096, 4096), "256x512": (256, 512, 512)}
CASES = [("ks%s_%dbit" % (shape, bits), group) for shape in SHAPES for bits in (32, 1) for group in (4, 8, 16)] + \
    [("enc%s_%dbit" % (shape, bits), 0) for shape in SHAPES for bits in (32, 1)]
CASE_SECONDS, SETUP_SECONDS, STEP_SECONDS = 900, 150, 60
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))  # PNG specification 8.2


def split_numpy(rows, w, bits):
    """raw scanlines (h, row_bytes) of one image -> its present passes back to back (no filter bytes), by the table"""
    import numpy as np
    px = rows.reshape(rows.shape[0], w, bits // 8) if bits >= 8 else np.unpackbits(rows, axis=1)[:, :w]
    out = []
    for xs, ys, xst, yst in ADAM7:
        sub = px[ys::yst, xs::xst]
        if sub.shape[0] and sub.shape[1]:
            out.append((np.ascontiguousarray(sub).reshape(sub.shape[0], -1) if bits >= 8 else np.packbits(sub, axis=1)).reshape(-1))
    return np.concatenate(out)


def parse(case):
    shape, bits = case[3 if case.startswith("enc") else 2:].split("_")
    return SHAPES[shape] + (int(bits[:-3]),)


def run_ks(case, reps):
    import torch
    from zlibstream_amd import Engine, png_adam7_split_batch_device, png_idat_layout
    n, w, h, bits = parse(case)
    with step_limit(SETUP_SECONDS, case, "setup"):
        eng = Engine(0)
        stream = torch.cuda.Stream()
        _, rb7, rows7 = png_idat_layout(w, h, bits, 1)
        rb = (w * bits + 7) // 8
        n_in, n_out = h * rb, sum(b * r for b, r in zip(rb7, rows7))
        d_in = [torch.randint(0, 256, (n_in,), dtype=torch.uint8, device="cuda") for _ in range(n)]
        d_out = [torch.zeros(n_out, dtype=torch.uint8, device="cuda") for _ in range(n)]
        d_copy = [torch.zeros(n_out, dtype=torch.uint8, device="cuda") for _ in range(n)]
        args = ([t.data_ptr() for t in d_in], [w] * n, [h] * n, [bits] * n, [t.data_ptr() for t in d_out])
        torch.cuda.synchronize()

    def split():
        png_adam7_split_batch_device(eng, *args, stream=stream.cuda_stream)

    def copy():
        for i in range(n):
            d_copy[i].copy_(d_in[i][:n_out], non_blocking=True)

    row = {"case": case, "group": os.environ.get("ZS_PNG_SPLIT_GROUP", "default"), "images": n, "bits": bits, "out_bytes": n * n_out, "reps": reps}
    with torch.cuda.stream(stream):
        with step_limit(STEP_SECONDS, case, "check"):
            split()
            stream.synchronize()
            exact = split_numpy(d_in[n - 1].cpu().numpy().reshape(h, rb), w, bits).tobytes() == d_out[n - 1].cpu().numpy().tobytes()
            row["split is the table's"] = exact
        with step_limit(STEP_SECONDS, case, "split"):
            eng.set_profiling(True)
            split(), split()
            times = []
            for _ in range(reps):
                split()
                times.append(eng.stage_ms()["png_split"])
            eng.set_profiling(False)
            ms = statistics.median(times)
            row["split_ms"], row["split_GBps"] = round(ms, 4), round(n * n_out / ms / 1e6, 2)
        with step_limit(STEP_SECONDS, case, "copy"):
            ms = median_ms(copy, stream, reps)
            row["copy_ms"], row["copy_GBps"] = round(ms, 4), round(n * n_out / ms / 1e6, 2)
    row["split_over_copy"] = round(row["split_ms"] / row["copy_ms"], 2)
    print(json.dumps(row), flush=True)
    return 0 if exact else 1


def run_encode(case, reps):
    import numpy as np
    import torch
    from zlibstream_amd import Engine, deflate_bound, png_decode_files_batch, png_encode_interlace_batch_device, png_file_bound, png_idat_layout
    n, w, h, bits = parse(case)
    depth, color = (8, 6) if bits == 32 else (1, 0)
    rb = (w * bits + 7) // 8
    with step_limit(SETUP_SECONDS, case, "setup"):
        eng = Engine(0)
        imgs = [np.frombuffer(noisy_gradient(rb, h, 100 + i), dtype=np.uint8) for i in range(min(n, 4))]
        d_px = [torch.from_numpy(imgs[i % len(imgs)].copy()).cuda() for i in range(n)]
        cap = png_file_bound(deflate_bound(png_idat_layout(w, h, bits, 1)[0]), 0, 0)
        d_out = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
        d_back = torch.zeros(h * rb, dtype=torch.uint8, device="cuda")
        px, out = [t.data_ptr() for t in d_px], [t.data_ptr() for t in d_out]
        torch.cuda.synchronize()
    lens = {}

    def encode(il, rows_per_write=1):
        lens[il] = png_encode_interlace_batch_device(eng, px, [w] * n, [h] * n, [depth] * n, [color] * n, [5] * n, out, [cap] * n, interlace=[il] * n,
                                                     rows_per_write=rows_per_write, level=6)

    row = {"case": case, "images": n, "bits": bits, "pixel_bytes": n * h * rb, "level": 6, "reps": reps}
    with step_limit(2 * STEP_SECONDS, case, "check"):
        encode(1)
        torch.cuda.synchronize()
        f = d_out[n - 1][:lens[1][n - 1]].cpu().numpy().tobytes()
        st, info = png_decode_files_batch(eng, [f], [d_back.data_ptr()], [h * rb])
        exact = st == [0] and info[0]["interlace"] == 1 and torch.equal(d_back, d_px[n - 1])
        row["the decoder gives the pixels back"] = exact
    for il in (1, 0):
        # (a Write per row of a narrow pass can put a stream on the one-wave literal engine: seconds a call)
        with step_limit(5 * STEP_SECONDS, case, "interlace %d" % il):
            row["interlace%d_ms" % il] = round(wall_ms(lambda: encode(il), reps), 3)
            row["interlace%d_file_bytes" % il] = int(sum(lens[il]))
        with step_limit(2 * STEP_SECONDS, case, "interlace %d, one Write" % il):
            row["interlace%d_one_write_ms" % il] = round(wall_ms(lambda: encode(il, 0), reps), 3)
    with step_limit(STEP_SECONDS, case, "stages"):
        eng.set_profiling(True)
        encode(1)
        row["interlace1_stage_ms"] = {k: round(v, 3) for k, v in eng.stage_ms().items() if v > 0}
        eng.set_profiling(False)
    row["interlace1_over_interlace0"] = round(row["interlace1_ms"] / row["interlace0_ms"], 3)
    row["interlace1_over_interlace0_one_write"] = round(row["interlace1_one_write_ms"] / row["interlace0_one_write_ms"], 3)
    print(json.dumps(row), flush=True)
    return 0 if exact else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_interlace.log"))
    a = ap.parse_args()
    if a.case:
        sys.exit((run_ks if a.case.startswith("ks") else run_encode)(a.case, a.reps))
    lines, failed = [], False
    for case, group in CASES:
        env = dict(os.environ)
        env.pop("ZS_PNG_SPLIT_GROUP", None)
        if group:
            env["ZS_PNG_SPLIT_GROUP"] = str(group)
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
