"""The batched PNG encoder (zs_deflate_writes_batch_device, zs_png_filter_batch_device, zs_png_idat_batch_device), the parts
that need no GPU: the entries exist at every layer, reject bad arguments before any device call, and the host logic behind
them -- the packing of the streams' Write lists and the row-to-image lookup of the batch filter kernel -- does what the
device code relies on, run on the host from the headers the library compiles."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS_STREAM_ERROR = -2
NAMES = ("zs_deflate_writes_batch_device", "zs_png_filter_batch_device", "zs_png_idat_batch_device")


def test_entry_points_resolve_at_every_layer():
    from zlibstream_amd import _native, build
    L = ctypes.CDLL(build.build_engine())
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _native.SYMBOLS, name
    import zlibstream_amd
    assert callable(zlibstream_amd.Engine.deflate_writes_batch_device)
    assert callable(zlibstream_amd.png_filter_batch_device) and callable(zlibstream_amd.png_idat_batch_device)
    for f in ("include/zsgpu.hpp", "dotnet/ZsGpu.cs"):
        text = open(os.path.join(ROOT, f)).read()
        for name in NAMES:
            assert name in text, (f, name)


def test_a_null_context_is_a_stream_error_whatever_else_is_passed():
    from zlibstream_amd import _native
    L = _native.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    VP, I64, I32 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_int * 1
    P64 = ctypes.POINTER(ctypes.c_int64)
    ends = (ctypes.c_int64 * 2)(10, 64)
    lists = (P64 * 1)(ctypes.cast(ends, P64))
    olen, st = I64(7), I32(7)
    for n in (-1, 0, 1):
        for level in (6, 99):
            assert L.zs_deflate_writes_batch_device(None, n, VP(p), I64(64), lists, I64(2), VP(p), I64(256), olen, st, level, 0, 0, None) == ZS_STREAM_ERROR
            assert L.zs_deflate_writes_batch_device(None, n, VP(p), I64(64), None, None, VP(p), I64(256), olen, st, level, 0, 0, None) == ZS_STREAM_ERROR
        for row_bytes, height, bpp, ftype in ((4, 2, 1, 5), (4, 2, 0, 0), (4, 2, 9, 0), (0, 2, 1, 0), (4, 0, 1, 0), (4, 2, 1, 6), (4, 2, 1, -1)):
            assert L.zs_png_filter_batch_device(None, n, VP(p), I64(row_bytes), I64(height), I32(bpp), I32(ftype), VP(p), None) == ZS_STREAM_ERROR
            for rows_per_write in (-1, 0, 1):
                assert L.zs_png_idat_batch_device(None, n, VP(p), I64(row_bytes), I64(height), I32(bpp), I32(ftype), rows_per_write, VP(p), I64(256),
                                                  olen, st, 6, 0, 0, None) == ZS_STREAM_ERROR
    assert L.zs_png_filter_batch_device(None, 1, None, None, None, None, None, None, None) == ZS_STREAM_ERROR
    assert L.zs_png_idat_batch_device(None, 1, None, None, None, None, None, 1, None, None, None, None, 6, 0, 0, None) == ZS_STREAM_ERROR


class NoEngine:  # the checks come before the engine is touched
    @property
    def handle(self):
        raise AssertionError("the engine was reached")

    _h = property(handle.fget)
    _lib = property(handle.fget)


def test_python_layer_raises_value_error_for_bad_arguments():
    from zlibstream_amd import Engine, png_filter_batch_device, png_idat_batch_device
    writes = Engine.deflate_writes_batch_device
    e = NoEngine()
    # lists of unequal length
    with pytest.raises(ValueError):
        writes(e, [4096, 4096], [100], [None, None], [8192, 8192], [200, 200])
    with pytest.raises(ValueError):
        writes(e, [4096, 4096], [100, 100], [None], [8192, 8192], [200, 200])
    with pytest.raises(ValueError):
        writes(e, [4096], [100], [[50, 100]], [8192, 8192], [200])
    # decreasing ends; a last end that is not in_len (in any stream of the batch)
    with pytest.raises(ValueError):
        writes(e, [4096], [100], [[60, 50, 100]], [8192], [200])
    with pytest.raises(ValueError):
        writes(e, [4096, 4096], [100, 100], [[50, 100], [10, 5, 100]], [8192, 8192], [200, 200])
    with pytest.raises(ValueError):
        writes(e, [4096], [100], [[50, 99]], [8192], [200])
    with pytest.raises(ValueError):
        writes(e, [4096], [100], [[50, 101]], [8192], [200])
    with pytest.raises(ValueError):
        writes(e, [4096, 4096], [100, 100], [None, (ctypes.c_int64 * 2)(50, 90)], [8192, 8192], [200, 200])
    # the filter and the composition: bpp outside 1..8, filter outside 0..5, negative rows_per_write, unequal lists
    for row_bytes, height, bpp, ftype in ((4, 2, 0, 0), (4, 2, 9, 0), (4, 2, 1, 6), (4, 2, 1, -1), (0, 2, 1, 0), (4, 0, 1, 0), (4, 1 << 31, 4, 0)):
        with pytest.raises(ValueError):
            png_filter_batch_device(e, [4096], [row_bytes], [height], [bpp], [ftype], [8192])
        with pytest.raises(ValueError):
            png_idat_batch_device(e, [4096], [row_bytes], [height], [bpp], [ftype], [8192], [200])
    with pytest.raises(ValueError):
        png_idat_batch_device(e, [4096], [4], [2], [1], [5], [8192], [200], rows_per_write=-1)
    with pytest.raises(ValueError):
        png_filter_batch_device(e, [4096, 4096], [4], [2], [1], [5], [8192])
    with pytest.raises(ValueError):
        png_idat_batch_device(e, [4096], [4], [2], [1], [5], [8192], [200, 200])
    with pytest.raises(ValueError):
        png_filter_batch_device(e, [0], [4], [2], [1], [5], [8192])
    with pytest.raises(ValueError):  # more than 2^31 - 1 rows in one call
        png_filter_batch_device(e, [4096, 4096], [4, 4], [(1 << 31) - 1, 1], [1, 1], [5, 5], [8192, 8192])


def test_an_empty_batch_returns_an_empty_result():
    from zlibstream_amd import Engine, png_filter_batch_device, png_idat_batch_device
    e = NoEngine()
    assert Engine.deflate_writes_batch_device(e, [], [], [], [], []) == []
    assert Engine.deflate_writes_batch_device(e, [], [], None, [], []) == []
    assert Engine.deflate_writes_batch_device(e, [], [], [], [], [], return_status=True) == (0, [], [])
    assert png_filter_batch_device(e, [], [], [], [], [], []) is None
    assert png_idat_batch_device(e, [], [], [], [], [], [], []) == []


def test_write_list_packer_and_row_lookup_on_the_host():
    """tests/cpp/test_writes_batch.cpp: zs_core.h write_list_ends / layout_write_blocks on 5000 random schedules -- empty Writes
    dropped, at most one distinct end collapsing to one Write, the streams' blocks of the device table 8-byte aligned and
    disjoint, every malformed list (a last end beyond or short of the input, decreasing ends, a negative end, no Writes for a
    non-empty input) rejected -- and zs_png.h png_row_image against a linear scan, heights of 1 and totals beyond 2^16 rows."""
    exe = os.path.join(ROOT, "build", "test_writes_batch")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_writes_batch.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-2000:]
