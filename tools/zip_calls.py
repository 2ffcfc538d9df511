#!/usr/bin/env python3
"""The ZIP calls on one MI355X beside the raw deflate calls they are built on: one call of each direction over the Canterbury
corpus of tests/golden/corpus as one archive, and over 64 archives of one 1 MiB text entry each; beside each the same buffers
through zs_deflate_wrap_batch_device / zs_inflate_wrap_batch_device with ZS_WRAP_RAW.  What the ZIP call costs over the raw
one is the upload of the files (decode), KC over the outputs, the framing copy and KZ.
Every figure is the median of --repeats timed calls behind a warm-up call, the variants of a group taken in turn inside every
repeat so that a drift of the machine meets all of them; the spread (min .. max) stands beside it.  A host clock around calls
that synchronise their stream; every timed call is the C entry point on argument arrays made beforehand.
usage: python tools/zip_calls.py [--archives 64] [--entry-bytes 1048576] [--repeats 9] [--level 6]
Prints one JSON line per group; fails without a GPU."""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from zlibstream_amd import Engine, WRAP_RAW, ZIP_AUTO, _native, datagen, wrap_bound, zip_bound, zip_file_info  # noqa: E402
from zlibstream_amd.api import _zip_puts  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--archives", type=int, default=64)
ap.add_argument("--entry-bytes", type=int, default=1 << 20)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--level", type=int, default=6)
a = ap.parse_args()
eng = Engine(0)
LIB = _native.lib()


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


def dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def arr(kind, values):
    return (kind * max(len(values), 1))(*values)


def group(title, archives):
    """archives: a list of lists of (name bytes, data bytes)."""
    flat = [d for arch in archives for _, d in arch]
    d_data = [dev(d) if d else None for d in flat]
    ptr = [t.data_ptr() if t is not None else 0 for t in d_data]
    sizes = [len(d) for d in flat]
    n, m = len(archives), len(flat)
    # ---- encode: the ZIP call, and raw deflate of the same buffers
    it = iter(zip(ptr, sizes))
    built = [_zip_puts([(name,) + next(it) + (ZIP_AUTO,) for name, _ in arch]) for arch in archives]
    bounds = [zip_bound([(name, 256, len(d)) for name, d in arch]) for arch in archives]
    z_out = [torch.empty(b, dtype=torch.uint8, device="cuda") for b in bounds]
    rows = (ctypes.POINTER(_native.ZipPut) * n)(*[ctypes.cast(p, ctypes.POINTER(_native.ZipPut)) for p, _ in built])
    counts, z_ptrs, z_caps = arr(ctypes.c_int, [len(x) for x in archives]), arr(ctypes.c_void_p, [t.data_ptr() for t in z_out]), arr(ctypes.c_int64, bounds)
    z_len, z_st = (ctypes.c_int64 * n)(), (ctypes.c_int * n)()
    r_caps = [wrap_bound(s, WRAP_RAW) for s in sizes]
    r_out = [torch.empty(c, dtype=torch.uint8, device="cuda") for c in r_caps]
    r_in, r_in_len = arr(ctypes.c_void_p, ptr), arr(ctypes.c_int64, sizes)
    r_ptrs, r_capv, r_len, r_st = arr(ctypes.c_void_p, [t.data_ptr() for t in r_out]), arr(ctypes.c_int64, r_caps), (ctypes.c_int64 * m)(), (ctypes.c_int * m)()

    def zip_encode():
        rc = LIB.zs_zip_encode_batch_device(eng.handle, n, rows, counts, z_ptrs, z_caps, z_len, z_st, a.level, 0, 0, None)
        assert rc == 0, eng.last_error()

    def raw_deflate():
        rc = LIB.zs_deflate_wrap_batch_device(eng.handle, m, r_in, r_in_len, r_ptrs, r_capv, r_len, r_st, a.level, 0, 0, WRAP_RAW, None)
        assert rc == 0, eng.last_error()
    enc = timed({"zs_zip_encode_batch_device": zip_encode, "zs_deflate_wrap_batch_device_raw": raw_deflate})
    files = [bytes(t[:k].cpu().numpy()) for t, k in zip(z_out, z_len)]
    ok = True
    for f, arch in zip(files, archives):
        with zipfile.ZipFile(io.BytesIO(f)) as z:
            ok = ok and z.testzip() is None and [z.read(i) for i in z.infolist()] == [d for _, d in arch]
    # ---- decode: the ZIP call on the files in host memory, and raw inflate of the bodies where the encoder left them
    infos = [zip_file_info(f) for f in files]
    o_caps = [info["total_len"] for info, _ in infos]
    o_out = [torch.empty(max(c, 1), dtype=torch.uint8, device="cuda") for c in o_caps]
    keep = [ctypes.create_string_buffer(f, len(f)) for f in files]
    f_ptrs, f_lens = arr(ctypes.c_void_p, [ctypes.addressof(k) for k in keep]), arr(ctypes.c_int64, [len(f) for f in files])
    o_ptrs, o_capv, o_len, o_st = arr(ctypes.c_void_p, [t.data_ptr() for t in o_out]), arr(ctypes.c_int64, o_caps), (ctypes.c_int64 * n)(), (ctypes.c_int * n)()
    b_in, b_len, b_out, b_cap = [], [], [], []
    for t, o, (info, ents) in zip(z_out, o_out, infos):
        for e in ents:
            if e["method"] == 8:
                b_in.append(t.data_ptr() + e["body_off"]), b_len.append(e["comp_len"]), b_out.append(o.data_ptr() + e["out_off"]), b_cap.append(e["len"])
    k = len(b_in)
    bi, bl, bo, bc = arr(ctypes.c_void_p, b_in), arr(ctypes.c_int64, b_len), arr(ctypes.c_void_p, b_out), arr(ctypes.c_int64, b_cap)
    bol, bus, bst = (ctypes.c_int64 * max(k, 1))(), (ctypes.c_int64 * max(k, 1))(), (ctypes.c_int * max(k, 1))()

    def zip_decode():
        rc = LIB.zs_zip_decode_files_batch(eng.handle, n, f_ptrs, f_lens, o_ptrs, o_capv, o_len, None, o_st, None)
        assert rc == 0, eng.last_error()

    def raw_inflate():
        rc = LIB.zs_inflate_wrap_batch_device(eng.handle, k, bi, bl, bo, bc, bol, bus, bst, WRAP_RAW, None)
        assert rc == 0, eng.last_error()
    dec = timed({"zs_zip_decode_files_batch": zip_decode, "zs_inflate_wrap_batch_device_raw": raw_inflate})
    zip_decode()
    torch.cuda.synchronize()
    ok = ok and [bytes(o[:c].cpu().numpy()) for o, c in zip(o_out, o_caps)] == [b"".join(d for _, d in arch) for arch in archives]
    total = sum(sizes)
    for v in enc.values():
        v["MBps_in"] = round(total / v["ms_median"] / 1e3, 1)
    for v in dec.values():
        v["MBps_out"] = round(total / v["ms_median"] / 1e3, 1)
    print(json.dumps({"group": title, "archives": n, "entries": m, "deflated_entries": k, "bytes": total, "archive_bytes": sum(len(f) for f in files), "level": a.level,
                      "repeats": a.repeats, "round_trip": bool(ok), "encode": enc, "decode": dec,
                      "encode_extra_ms": round(enc["zs_zip_encode_batch_device"]["ms_median"] - enc["zs_deflate_wrap_batch_device_raw"]["ms_median"], 3),
                      "decode_extra_ms": round(dec["zs_zip_decode_files_batch"]["ms_median"] - dec["zs_inflate_wrap_batch_device_raw"]["ms_median"], 3)}))


corpus_dir = os.path.join(ROOT, "tests", "golden", "corpus")
corpus = [(name.encode(), open(os.path.join(corpus_dir, name), "rb").read()) for name in sorted(os.listdir(corpus_dir))]
group("the Canterbury corpus as one archive", [corpus])
text = datagen.english(a.archives * a.entry_bytes, datagen.GOLDEN)
group("%d archives of one text entry of %d bytes" % (a.archives, a.entry_bytes),
      [[(b"entry%03d.txt" % i, bytes(text[i * a.entry_bytes:(i + 1) * a.entry_bytes]))] for i in range(a.archives)])
