#!/usr/bin/env python3
"""The container calls on one MI355X: zlib, raw and gzip inflate of the same level-6 text body, BGZF-sized gzip members,
and deflate into the three containers.  Every figure is the median of --repeats timed calls behind a warm-up call, the
variants of a group taken in turn inside every repeat so that a drift of the machine meets all of them; the spread
(min .. max) stands beside it.  A host clock around calls that synchronise their stream.  Every timed call is the C entry
point on argument arrays made beforehand (turning Python lists of a thousand streams into C arrays costs as much as the
device takes for a tenth of such a batch).
usage: python tools/wrap_bench.py [--size 67108864] [--members 1024] [--repeats 7] [--parent-lib PATH]
--parent-lib: another build of the library (the commit before); its zs_inflate_batch_device and zs_deflate_batch_device run
in the same turns on the same buffers.  Prints one JSON line per group."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from zlibstream_amd import Engine, WRAP_GZIP, WRAP_RAW, WRAP_ZLIB, _native, datagen, deflate_wrap_batch_device, wrap_bound  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=64 << 20)
ap.add_argument("--members", type=int, default=1024)
ap.add_argument("--member-bytes", type=int, default=65280)  # what bgzip puts into a block
ap.add_argument("--deflate-streams", type=int, default=16)
ap.add_argument("--deflate-bytes", type=int, default=4 << 20)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--parent-lib", default=None)
a = ap.parse_args()
eng = Engine(0)
WRAPS = (("zlib", WRAP_ZLIB), ("raw", WRAP_RAW), ("gzip", WRAP_GZIP))


class Parent:
    """The batch calls of another build of the library, on a context of its own."""

    def __init__(self, path):
        self.L = L = ctypes.CDLL(path)
        vp, i32, i64, P = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.POINTER
        L.zs_ctx_create.argtypes = [i32, P(vp)]
        L.zs_inflate_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(vp), P(i64), P(i64), P(i32), vp]
        L.zs_deflate_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(vp), P(i64), P(i64), P(i32), i32, i32, i32, vp]
        self.h = vp()
        if L.zs_ctx_create(0, ctypes.byref(self.h)) != 0:
            raise RuntimeError("the parent library found no device")


parent = Parent(a.parent_lib) if a.parent_lib else None
LIB = _native.lib()


class Args:
    """The argument arrays of a batch call as C arrays, made once."""

    def __init__(self, ins, in_lens, outs, caps):
        n = self.n = len(ins)
        self.ins, self.in_lens = (ctypes.c_void_p * n)(*ins), (ctypes.c_int64 * n)(*in_lens)
        self.outs, self.caps = (ctypes.c_void_p * n)(*outs), (ctypes.c_int64 * n)(*caps)
        self.out_len, self.in_used, self.status = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)(), (ctypes.c_int * n)()


def timed(variants):
    """variants: {name: callable}.  One warm-up call each, then --repeats turns through all of them."""
    for f in variants.values():
        f()
    times = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)} for k, v in times.items()}


def deflate_into(datas, wrap, level=6):
    """-> (device tensors, lengths) of the streams of `datas` (device tensors) in container `wrap`."""
    caps = [wrap_bound(d.numel(), wrap) for d in datas]
    outs = [torch.empty(c, dtype=torch.uint8, device="cuda") for c in caps]
    rc, lens, status = deflate_wrap_batch_device(eng, [d.data_ptr() for d in datas], [d.numel() for d in datas], [o.data_ptr() for o in outs], caps, wrap, level)
    assert rc == 0, eng.last_error()
    return outs, lens


def inflate_group(title, datas):
    sizes = [d.numel() for d in datas]
    outs = [torch.empty(max(s, 1), dtype=torch.uint8, device="cuda") for s in sizes]
    forms = {name: deflate_into(datas, w) for name, w in WRAPS}
    args = {name: Args([t.data_ptr() for t in forms[name][0]], forms[name][1], [o.data_ptr() for o in outs], sizes) for name, _ in WRAPS}

    def run(name, w):
        g = args[name]

        def f():
            rc = LIB.zs_inflate_wrap_batch_device(eng.handle, g.n, g.ins, g.in_lens, g.outs, g.caps, g.out_len, g.in_used, g.status, w, None)
            assert rc == 0, eng.last_error()
        return f
    variants = {name: run(name, w) for name, w in WRAPS}
    g0 = args["zlib"]

    def plain():
        assert LIB.zs_inflate_batch_device(eng.handle, g0.n, g0.ins, g0.in_lens, g0.outs, g0.caps, g0.out_len, g0.status, None) == 0
    variants["zs_inflate_batch_device"] = plain
    if parent:
        def old():
            assert parent.L.zs_inflate_batch_device(parent.h, g0.n, g0.ins, g0.in_lens, g0.outs, g0.caps, g0.out_len, g0.status, None) == 0
        variants["parent_zs_inflate_batch_device"] = old
    res = timed(variants)
    ok = all(torch.equal(o[:s], d) for o, s, d in zip(outs, sizes, datas))
    ok = ok and all(list(args[name].out_len) == sizes and list(args[name].in_used) == forms[name][1] for name, _ in WRAPS)
    total = sum(sizes)
    for v in res.values():
        v["MBps_out"] = round(total / v["ms_median"] / 1e3, 1)
    print(json.dumps({"group": title, "streams": len(datas), "bytes_out": total, "repeats": a.repeats, "round_trip": ok, **res}))


def deflate_group(title, datas):
    sizes = [d.numel() for d in datas]
    variants, keep = {}, []
    for name, w in WRAPS:
        caps = [wrap_bound(s, w) for s in sizes]
        outs = [torch.empty(c, dtype=torch.uint8, device="cuda") for c in caps]
        keep.append(outs)
        g = Args([d.data_ptr() for d in datas], sizes, [o.data_ptr() for o in outs], caps)

        def f(w=w, g=g):
            rc = LIB.zs_deflate_wrap_batch_device(eng.handle, g.n, g.ins, g.in_lens, g.outs, g.caps, g.out_len, g.status, 6, 0, 0, w, None)
            assert rc == 0, eng.last_error()
        variants[name] = f
        if w == WRAP_ZLIB and parent:
            def old(g=g):
                assert parent.L.zs_deflate_batch_device(parent.h, g.n, g.ins, g.in_lens, g.outs, g.caps, g.out_len, g.status, 6, 0, 0, None) == 0
            variants["parent_zs_deflate_batch_device"] = old
    res = timed(variants)
    total = sum(sizes)
    for v in res.values():
        v["MBps_in"] = round(total / v["ms_median"] / 1e3, 1)
    print(json.dumps({"group": title, "streams": len(datas), "bytes_in": total, "repeats": a.repeats, **res}))


def dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


text = datagen.english(a.size, datagen.GOLDEN)
inflate_group("inflate: one level-6 text body of %d bytes" % a.size, [dev(text)])
mb = a.member_bytes
inflate_group("inflate: %d members of %d bytes (BGZF-sized)" % (a.members, mb), [dev(text[(i * mb) % (len(text) - mb):][:mb]) for i in range(a.members)])
db = a.deflate_bytes
deflate_group("deflate, level 6: %d streams of %d bytes" % (a.deflate_streams, db), [dev(text[(i * db) % max(len(text) - db, 1):][:db]) for i in range(a.deflate_streams)])
