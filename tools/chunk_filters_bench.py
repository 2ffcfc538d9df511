#!/usr/bin/env python3
"""The chunk filters on one MI355X: 256 chunks of 1 MiB of int32 (an 8192 x 8192 array in chunks of 512 x 512), smooth data from
tests/chunk_cases.py smooth_array (sixteen pieces of 16 MiB, seeds 1..16), shuffle on, zlib level 6.
  calls     zs_chunks_encode_batch_device and zs_chunks_decode_batch -- the calls without filters, the baseline -- beside the two
            _filters_ calls with every filter 0, with each filter alone and with all three.  A host clock around calls that
            synchronise their stream.  `added_ms` is a variant's median less the baseline's, `floor_ms` the time the filter's own
            device traffic would take at 6.3 TB/s, the copy rate the HBM reaches (8 TB/s is its specification): for Fletcher-32
            the stored bytes read once; for delta on decode the chunk bytes read twice and written once, and read once more by
            the place kernel, less the one read and one write that the fused place makes without it: two reads and a write more,
            on encode one read and one write more; the byte order adds no traffic.
  stages    one profiled call of each variant (zs_ctx_set_profiling: device events around every stage): the chunk stage -- KN, and
            with filters KL's tile launch and KI's launches -- and the sum of the other stages (deflate or inflate, KC).  Delta
            changes the bytes that deflate and inflate work on, so a call's time moves with the codec; `added_chunk_stage_ms` is
            what the filter's own launches add, beside the same floors.
  kernels   the stand-alone calls on the 256 chunk-sized buffers: zs_fletcher32_batch_device, zs_delta_encode_batch_device,
            zs_delta_decode_batch_device, by device events around their launches (zs_ctx_set_profiling, stage "chunk_kn": for
            Fletcher-32 the tile launch, for delta all of them) and by the host clock around the call; GB/s counts the bytes
            read plus written (Fletcher-32: read).
Every figure is the median of --repeats behind a warm-up, the variants of a group taken in turn; min .. max beside it.
usage: python tools/chunk_filters_bench.py [--repeats 7] [--level 6] [--out profiles/chunk_filters_times.log]
Prints one JSON line per group and writes them to --out; fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import chunk_cases as cc  # noqa: E402
from zlibstream_amd import (Engine, chunk_grid_info, chunks_decode, chunks_encode, chunks_filters_bound, delta_decode, delta_encode,  # noqa: E402
                            fletcher32)

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--level", type=int, default=6)
ap.add_argument("--out", default=None)
a = ap.parse_args()
eng = Engine(0)
HBM = 6.3e12  # bytes a second
grid = {"shape": (8192, 8192), "chunks": (512, 512), "elem_size": 4, "shuffle": True, "wrap": 0, "fill": bytes(4)}
n_chunks, chunk_bytes, array_bytes = chunk_grid_info(grid)
lines = []


def emit(d):
    lines.append(json.dumps(d))
    print(lines[-1], flush=True)


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


piece = cc.grid((1 << 22,), (1 << 18,), 4)
data = b"".join(cc.smooth_array(piece, 1 + k) for k in range(array_bytes // cc.array_bytes(piece)))
d_arr = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
d_back = torch.empty(array_bytes, dtype=torch.uint8, device="cuda")
VARIANTS = {"no_filters_call": None, "filters_all_0": dict(delta=0, byte_order=0, fletcher32=0), "fletcher32": dict(fletcher32=1), "delta": dict(delta=1),
            "byte_order": dict(byte_order=1), "all_three": dict(delta=1, byte_order=1, fletcher32=1)}
bound = max(chunks_filters_bound(grid, f or {}) for f in VARIANTS.values())
d_out = torch.empty(bound, dtype=torch.uint8, device="cuda")


def enc(f):
    rc, lens, tables, status = chunks_encode(eng, [grid], [d_arr.data_ptr()], [d_out.data_ptr()], [bound], level=a.level, filters=None if f is None else [f])
    assert rc == 0
    return lens[0], tables[0]


stored, chunks = {}, {}
for name, f in VARIANTS.items():
    total, table = enc(f)
    host = d_out[:total].cpu().numpy().tobytes()
    stored[name], chunks[name] = total, [host[off:off + ln] for off, ln, _ in table]


def dec(name):
    f = VARIANTS[name]
    rc, codes, status = chunks_decode(eng, [grid], [chunks[name]], [d_back.data_ptr()], [array_bytes], filters=None if f is None else [f])
    assert rc == 0


for name in VARIANTS:
    d_back.zero_()
    dec(name)
    assert torch.equal(d_back, d_arr), "decode of encode is not the identity: " + name
emit({"group": "setup", "array_mib": array_bytes / 2**20, "chunks": n_chunks, "chunk_kib": chunk_bytes / 1024, "level": a.level,
      "stored_mib": {k: round(v / 2**20, 2) for k, v in stored.items()}, "clock": "host perf_counter around synchronised calls; device events for kernels",
      "hbm_bytes_per_s_for_floors": HBM})


def floors(side):
    ms = lambda b: round(b / HBM * 1e3, 3)  # noqa: E731
    delta = (3 if side == "decode" else 2) * array_bytes
    return {"filters_all_0": 0.0, "fletcher32": ms(stored["fletcher32"]), "delta": ms(delta), "byte_order": 0.0, "all_three": ms(stored["all_three"] + delta)}


for side, call in (("encode", lambda n: enc(VARIANTS[n]) and None), ("decode", dec)):
    t = timed({n: (lambda n=n: call(n)) for n in VARIANTS})
    base = t["no_filters_call"]["ms_median"]
    fl = floors(side)
    emit({"group": "calls_" + side, **t, "added_ms": {n: round(t[n]["ms_median"] - base, 3) for n in fl}, "floor_ms": fl})


def profiled(call):
    """the stages of one profiled call: KN, KL and KI together ("chunk_kn"), and every other stage (deflate or inflate, KC)"""
    eng.set_profiling(True)
    call()
    stages = eng.stage_ms()
    eng.set_profiling(False)
    return stages.get("chunk_kn", 0.0), sum(v for k, v in stages.items() if k != "chunk_kn")


# the filters' own launches by device events: what a variant's chunk stage takes more than the baseline's, beside the other
# stages -- deflate and inflate work on other bytes behind delta, and that difference is the codec's, not the filter's
for side, call in (("encode", lambda n: enc(VARIANTS[n])), ("decode", dec)):
    kn, rest = {n: [] for n in VARIANTS}, {n: [] for n in VARIANTS}
    for turn in range(a.repeats + 1):
        for n in VARIANTS:
            k, r = profiled(lambda n=n: call(n))
            if turn:
                kn[n].append(k), rest[n].append(r)
    base = statistics.median(kn["no_filters_call"])
    fl = floors(side)
    emit({"group": "stages_" + side, "chunk_stage": {n: spread(v) for n, v in kn.items()}, "other_stages": {n: spread(v) for n, v in rest.items()},
          "added_chunk_stage_ms": {n: round(statistics.median(kn[n]) - base, 3) for n in fl}, "floor_ms": fl,
          "added_over_floor": {n: round((statistics.median(kn[n]) - base) / fl[n], 2) for n in fl if fl[n] > 0}})

# the stand-alone kernels on chunk-sized buffers
d_b = torch.empty(array_bytes, dtype=torch.uint8, device="cuda")
pa, pb = [d_arr.data_ptr() + k * chunk_bytes for k in range(n_chunks)], [d_b.data_ptr() + k * chunk_bytes for k in range(n_chunks)]
sizes, ess = [chunk_bytes] * n_chunks, [4] * n_chunks


def kernel_ms(fn):
    eng.set_profiling(True)
    fn()
    ms = eng.stage_ms().get("chunk_kn", 0.0)
    eng.set_profiling(False)
    return ms


KERNELS = {"fletcher32": (lambda: fletcher32(eng, pa, sizes) and None, array_bytes), "delta_encode": (lambda: delta_encode(eng, pa, pb, sizes, ess), 2 * array_bytes),
           "delta_decode": (lambda: delta_decode(eng, pa, pb, sizes, ess), 3 * array_bytes)}
ev = timed({k: (lambda f=f: kernel_ms(f)) for k, (f, _) in KERNELS.items()})
host = timed({k: f for k, (f, _) in KERNELS.items()})
emit({"group": "kernels", "bytes": array_bytes, "device_events": ev, "host_clock_around_call": host,
      "gb_per_s_by_device_events": {k: round(b / (ev[k]["ms_median"] * 1e-3) / 1e9, 1) for k, (_, b) in KERNELS.items()},
      "floor_ms": {k: round(b / HBM * 1e3, 3) for k, (_, b) in KERNELS.items()},
      "over_floor": {k: round(ev[k]["ms_median"] / (b / HBM * 1e3), 2) for k, (_, b) in KERNELS.items()}})
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
