"""CRC-32 on the device and the cost of whole PNG files around the IDAT calls, everything but the decoder's input resident in HBM.

    crc32         zs_crc32_device on one 64 MiB buffer; zs_crc32_batch_device on 8192 x 8 KiB and on 64 x 1 MiB spans of it
    adler32       zs_adler32_device on the same 64 MiB (the project's nearest one-pass read-only reduction)
    zlib          zlib.crc32 on one host core over the same bytes
    encode        zs_png_encode_batch_device against zs_png_idat_batch_device on identical input: the difference is the framing
    decode        zs_png_decode_files_batch (files in host memory) against zs_png_decode_batch_device on the payloads already
                  gathered on the device: the difference is staging, the CRC check and the gather

encode / decode: 64 images of 1024 x 1024 RGBA (noisy gradients), adaptive filter, one Write per image, levels 1 and 6.
Wall-clock milliseconds around calls that end in the call's own wait for its stream, the device idle before; every leg is
warmed up once, then the legs of a pair alternate --runs times: median and spread (max - min).  Rates are bytes of the spans
over the wall time of the call (one launch pair, one upload of descriptors, one wait), "kernel" the two launches alone by
device events (zs_ctx_stage_ms "crc32_frame") in calls of their own.  ZS_CRC32_FORM=1 selects the kernel's staged form.

    python tools/png_file_bench.py [--runs 7] [--out profiles/png_file.log]
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def noisy_gradient(row_bytes, height, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    grad = (np.add.outer(np.arange(height) * 3, np.arange(row_bytes)) % 253).astype(np.uint8)
    return (grad + rng.integers(0, 4, grad.shape, dtype=np.uint8)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--crc-only", action="store_true", help="leave out the encode and decode legs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_file.log"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from zlibstream_amd import (Engine, _native, crc32_batch_device, crc32_device, deflate_bound, png_decode_batch_device, png_decode_files_batch,
                                png_encode_batch_device, png_file_bound, png_idat_batch_device)
    import ctypes
    if not torch.cuda.is_available():
        sys.exit("png_file_bench: no GPU (there is nothing to measure without one)")
    eng = Engine(0)
    L = _native.lib()
    lines = ["form: %s" % ("staged (ZS_CRC32_FORM=1)" if os.environ.get("ZS_CRC32_FORM") == "1" else "strided (default)")]

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3  # (every call here returns after its own wait for the stream)

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}

    def pair(legs, runs):
        """alternating runs of the named legs -> name -> list of ms"""
        for fn in legs.values():
            timed(fn)
        out = {k: [] for k in legs}
        for _ in range(runs):
            for k, fn in legs.items():
                out[k].append(timed(fn))
        return out

    # ---------------------------------------------------------------- CRC-32 and Adler-32 over 64 MiB
    nbytes = a.mib << 20
    host = np.random.default_rng(1).integers(0, 256, nbytes, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    base = dev.data_ptr()
    want = zlib.crc32(host.tobytes())
    ad = ctypes.c_uint32(0)

    def adler():
        assert L.zs_adler32_device(eng.handle, ctypes.c_void_p(base), nbytes, 1, ctypes.byref(ad), None) == 0

    shapes = {"one_span": [(0, nbytes)], "8KiB_spans": [(i << 13, 1 << 13) for i in range(nbytes >> 13)], "1MiB_spans": [(i << 20, 1 << 20) for i in range(nbytes >> 20)]}
    got = {}
    legs = {"crc32_one_span": lambda: got.__setitem__("one", crc32_device(eng, base, nbytes)), "adler32": adler}
    for name in ("8KiB_spans", "1MiB_spans"):
        ptrs, lens = [base + s for s, _ in shapes[name]], [n for _, n in shapes[name]]
        legs["crc32_" + name] = lambda ptrs=ptrs, lens=lens, name=name: got.__setitem__(name, crc32_batch_device(eng, ptrs, lens))
    reps = 5
    res = pair({k: (lambda fn=fn: [fn() for _ in range(reps)]) for k, fn in legs.items()}, a.runs)
    assert got["one"] == want and ad.value == zlib.adler32(host.tobytes())
    hb = host.tobytes()
    for name in ("8KiB_spans", "1MiB_spans"):
        assert got[name] == [zlib.crc32(hb[s:s + n]) for s, n in shapes[name]], name
    for k, v in res.items():
        per = [x / reps for x in v]
        emit(dict({"leg": k, "bytes": nbytes, "calls_per_run": reps, "GBps_of_median": round(nbytes / statistics.median(per) / 1e6, 1)}, **stats(per)))
    eng.set_profiling(True)
    for name, fn in (("crc32_one_span", legs["crc32_one_span"]), ("crc32_8KiB_spans", legs["crc32_8KiB_spans"]), ("crc32_1MiB_spans", legs["crc32_1MiB_spans"])):
        ks = []
        for _ in range(a.runs):
            fn()
            ks.append(eng.stage_ms()["crc32_frame"])
        emit(dict({"leg": name + " kernel (device events)", "bytes": nbytes, "GBps_of_median": round(nbytes / statistics.median(ks) / 1e6, 1)}, **stats(ks)))
    eng.set_profiling(False)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        zlib.crc32(hb)
        t.append((time.perf_counter() - t0) * 1e3)
    emit(dict({"leg": "zlib.crc32, one host core", "bytes": nbytes, "GBps_of_median": round(nbytes / statistics.median(t) / 1e6, 2)}, **stats(t)))
    del dev

    # ---------------------------------------------------------------- files around the IDAT calls
    n, side = (0 if a.crc_only else a.images), a.side
    rb = 4 * side
    raw = [noisy_gradient(rb, side, 100 + i) for i in range(n)]
    d_px = [torch.from_numpy(x.reshape(-1)).cuda() for x in raw]
    zcap = deflate_bound(side * (rb + 1))
    fcap = png_file_bound(zcap, 8192, 0)
    d_z = [torch.zeros(zcap, dtype=torch.uint8, device="cuda") for _ in range(n)]
    d_f = [torch.zeros(fcap, dtype=torch.uint8, device="cuda") for _ in range(n)]
    d_out = [torch.zeros(side * rb, dtype=torch.uint8, device="cuda") for _ in range(n)]
    px, zp, fp, op = ([t.data_ptr() for t in x] for x in (d_px, d_z, d_f, d_out))
    torch.cuda.synchronize()
    for level in (1, 6) if n else ():
        for chunk in (0, 8192):
            state = {}

            def idat():
                state["zlen"] = png_idat_batch_device(eng, px, [rb] * n, [side] * n, [4] * n, [5] * n, zp, [zcap] * n, rows_per_write=0, level=level)

            def encode():
                state["flen"] = png_encode_batch_device(eng, px, [side] * n, [side] * n, [8] * n, [6] * n, [5] * n, fp, [fcap] * n, rows_per_write=0,
                                                        idat_chunk_bytes=chunk, level=level)

            res = pair({"idat": idat, "encode": encode}, a.runs)
            files = [d_f[i][:state["flen"][i]].cpu().numpy().tobytes() for i in range(n)]
            eng.set_profiling(True)
            encode()
            frame_ms = eng.stage_ms()["crc32_frame"]
            eng.set_profiling(False)
            mi, me = statistics.median(res["idat"]), statistics.median(res["encode"])
            emit({"leg": "encode", "level": level, "idat_chunk_bytes": chunk, "images": n, "pixel_bytes": n * side * rb, "stream_bytes": int(sum(state["zlen"])),
                  "idat": stats(res["idat"]), "encode": stats(res["encode"]), "framing_ms (encode - idat, medians)": round(me - mi, 4),
                  "framing share of idat": round((me - mi) / mi, 4), "framing launches by device events ms": round(frame_ms, 4)})
            if chunk:
                continue

            def decode_payloads():
                st = png_decode_batch_device(eng, zp, state["zlen"], [side] * n, [side] * n, [32] * n, [0] * n, op)
                assert st == [0] * n

            def decode_files():
                st, _ = png_decode_files_batch(eng, files, op, [side * rb] * n)
                assert st == [0] * n

            res = pair({"payloads": decode_payloads, "files": decode_files}, a.runs)
            assert all(torch.equal(x, y) for x, y in zip(d_out, d_px))
            eng.set_profiling(True)
            decode_files()
            check_ms = eng.stage_ms()["crc32_frame"]
            eng.set_profiling(False)
            mp, mf = statistics.median(res["payloads"]), statistics.median(res["files"])
            emit({"leg": "decode", "level": level, "images": n, "file_bytes": sum(len(f) for f in files), "payloads": stats(res["payloads"]), "files": stats(res["files"]),
                  "staging + check + gather ms (files - payloads, medians)": round(mf - mp, 4), "check + gather launches by device events ms": round(check_ms, 4)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
