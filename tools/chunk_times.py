#!/usr/bin/env python3
"""The chunked-array calls on one MI355X: a 256 MiB float32 array of smooth data in 1 MiB chunks (8192 x 8192 elements, chunks
of 512 x 512), shuffle on, zlib level 6, written by one zs_chunks_encode_batch_device call and read back by one
zs_chunks_decode_batch call.
  calls    the two calls, a host clock around calls that synchronise their stream
  stages   one profiled call of each (zs_ctx_set_profiling: device events around every stage): KN ("chunk_kn": the gather
           kernel, or the place kernel), the sum of the deflate or inflate stages, KC's span copy, and the rest of the call's
           time -- on the decode side the chunks' way up from host memory (the binding's copy, the staging copy, the upload)
  kernels  KN's time from those events beside a device-to-device copy of the array's bytes (torch's copy_ between two device
           buffers, a hipMemcpyAsync, by device events): the kernels move each byte once in and once out, as the copy does;
           and the filter alone on the 256 chunk-sized buffers (zs_shuffle_batch_device, zs_unshuffle_batch_device)
Every figure is the median of --repeats behind a warm-up, the variants of a group taken in turn; min .. max beside it.  Only the
fused place (unshuffle and placement in one pass) exists: a two-pass form was not built, so there is nothing to compare it with.
usage: python tools/chunk_times.py [--side 8192] [--chunk 512] [--repeats 7] [--level 6]
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
from zlibstream_amd import Engine, chunk_grid_info, chunks_bound, chunks_decode, chunks_encode, shuffle, unshuffle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=8192)
ap.add_argument("--chunk", type=int, default=512)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--level", type=int, default=6)
a = ap.parse_args()
eng = Engine(0)
S, C = a.side, a.chunk
grid = {"shape": (S, S), "chunks": (C, C), "elem_size": 4, "shuffle": True, "wrap": 0, "fill": bytes(4)}
n_chunks, chunk_bytes, array_bytes = chunk_grid_info(grid)


def spread(v):
    return {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}


def timed(variants):
    """variants: {name: callable returning None (host clock) or a time in ms}.  A warm-up each, then --repeats turns."""
    for f in variants.values():
        f()
    times = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ms = f()
            torch.cuda.synchronize()
            times[k].append(ms if ms is not None else (time.perf_counter() - t0) * 1e3)
    return {k: spread(v) for k, v in times.items()}


# smooth data: a field a simulation would leave, with a little noise in the low mantissa bits
y, x = np.mgrid[0:S, 0:S].astype(np.float32)
field = np.sin(x / 97.0) * np.cos(y / 131.0) + np.sin((x + y) / 411.0)
field += 1e-4 * np.random.default_rng(1).standard_normal((S, S), dtype=np.float32)
d_arr = torch.from_numpy(field.view(np.uint8).reshape(-1)).cuda()
del x, y
bound = chunks_bound(grid)
d_out = torch.empty(bound, dtype=torch.uint8, device="cuda")
d_back = torch.empty(array_bytes, dtype=torch.uint8, device="cuda")


def enc():
    rc, lens, tables, status = chunks_encode(eng, [grid], [d_arr.data_ptr()], [d_out.data_ptr()], [bound], level=a.level)
    assert rc == 0
    return lens[0], tables[0]


total, table = enc()
host = d_out[:total].cpu().numpy().tobytes()
chunks = [host[off:off + ln] for off, ln, _ in table]


def dec():
    rc, codes, status = chunks_decode(eng, [grid], [chunks], [d_back.data_ptr()], [array_bytes])
    assert rc == 0


dec()
assert torch.equal(d_back, d_arr), "decode of encode is not the identity"
print(json.dumps({"group": "setup", "array_mib": array_bytes / 2**20, "chunks": n_chunks, "chunk_kib": chunk_bytes / 1024, "compressed_mib": round(total / 2**20, 1),
                  "level": a.level}), flush=True)

print(json.dumps({"group": "calls", **timed({"chunks_encode": lambda: enc() and None, "chunks_decode": dec})}), flush=True)


def profiled(call):
    """the stages of one profiled call, and its time on the host clock"""
    eng.set_profiling(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    stages = {k: v for k, v in eng.stage_ms().items() if v > 0}
    eng.set_profiling(False)
    return ms, stages


def stage_report(call):
    profiled(call)
    runs = [profiled(call) for _ in range(a.repeats)]
    kn = [s["chunk_kn"] for _, s in runs]
    kc = [s.get("crc32_frame", 0.0) for _, s in runs]
    codec = [sum(v for k, v in s.items() if k not in ("chunk_kn", "crc32_frame")) for _, s in runs]
    rest = [ms - sum(s.values()) for ms, s in runs]
    return {"call_profiled": spread([ms for ms, _ in runs]), "chunk_kn": spread(kn), "deflate_or_inflate_stages": spread(codec), "kc_span_copy": spread(kc),
            "rest_upload_and_host": spread(rest)}, statistics.median(kn)


enc_stages, gather_ms = stage_report(enc)
dec_stages, place_ms = stage_report(dec)
print(json.dumps({"group": "stages_encode", **enc_stages}), flush=True)
print(json.dumps({"group": "stages_decode", **dec_stages}), flush=True)

# the filter alone on chunk-sized buffers, and the copy
d_a, d_b = torch.empty(n_chunks * chunk_bytes, dtype=torch.uint8, device="cuda"), torch.empty(n_chunks * chunk_bytes, dtype=torch.uint8, device="cuda")
d_a.copy_(d_arr[:d_a.numel()])
pa, pb = [d_a.data_ptr() + k * chunk_bytes for k in range(n_chunks)], [d_b.data_ptr() + k * chunk_bytes for k in range(n_chunks)]
sizes, ess = [chunk_bytes] * n_chunks, [4] * n_chunks


def kernel_ms(fn):
    eng.set_profiling(True)
    fn(eng, pa, pb, sizes, ess)
    ms = eng.stage_ms().get("chunk_kn", 0.0)
    eng.set_profiling(False)
    return ms


def copy_ms():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    d_back.copy_(d_arr)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


k = timed({"shuffle_alone": lambda: kernel_ms(shuffle), "unshuffle_alone": lambda: kernel_ms(unshuffle), "device_to_device_copy": copy_ms})
copy = k["device_to_device_copy"]["ms_median"]
print(json.dumps({"group": "kernels", "bytes": array_bytes, **k, "place_in_decode_ms": round(place_ms, 3), "gather_in_encode_ms": round(gather_ms, 3),
                  "place_over_copy": round(place_ms / copy, 2), "gather_over_copy": round(gather_ms / copy, 2),
                  "place_gb_per_s_read_plus_written": round(2 * array_bytes / (place_ms * 1e-3) / 1e9, 1),
                  "gather_gb_per_s_read_plus_written": round(2 * array_bytes / (gather_ms * 1e-3) / 1e9, 1)}), flush=True)
