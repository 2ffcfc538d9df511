"""PNG scanline reconstruction (zs_png_unfilter_device / zs_png_unfilter_batch_device), the parts that need no GPU: the entry
points exist at every layer and reject bad arguments before any device call, and the kernel's schedule -- run on the host with
the code the kernel compiles (zs_png.h) -- reconstructs what a plain row-by-row reading of PNG specification 9.2 gives."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS_STREAM_ERROR = -2


def test_entry_points_resolve_at_every_layer():
    from zlibstream_amd import _native, build
    L = ctypes.CDLL(build.build_engine())
    assert hasattr(L, "zs_png_unfilter_device") and hasattr(L, "zs_png_unfilter_batch_device")
    assert "zs_png_unfilter_device" in _native.SYMBOLS and "zs_png_unfilter_batch_device" in _native.SYMBOLS
    from zlibstream_amd import png_unfilter_device, png_unfilter_batch_device  # noqa: F401
    assert callable(png_unfilter_device) and callable(png_unfilter_batch_device)
    for f in ("include/zsgpu.hpp", "dotnet/ZsGpu.cs"):
        assert "zs_png_unfilter_device" in open(os.path.join(ROOT, f)).read(), f


def test_bad_arguments_are_rejected_before_any_device_call():
    """Without a GPU there is no context to pass, so this checks only that a null context is ZS_STREAM_ERROR whatever the other
    arguments are, and that no HIP call is needed to say so.  The checks of bpp, row_bytes, height and the pointers with a live
    context are in tests/test_gpu_png_unfilter.py (test_c_entry_points_reject_bad_arguments_with_a_real_context)."""
    from zlibstream_amd import _native
    L = _native.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    for row_bytes, height, bpp in ((4, 2, 1), (4, 2, 0), (4, 2, 9), (0, 2, 1), (4, 0, 1), (4, 1 << 31, 1)):
        assert L.zs_png_unfilter_device(None, p, row_bytes, height, bpp, p, None) == ZS_STREAM_ERROR
        VP, I64, I32 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_int * 1
        st = I32(7)
        assert L.zs_png_unfilter_batch_device(None, 1, VP(p), I64(row_bytes), I64(height), I32(bpp), VP(p), st, None) == ZS_STREAM_ERROR
    assert L.zs_png_unfilter_batch_device(None, 0, None, None, None, None, None, None, None) == ZS_STREAM_ERROR
    assert L.zs_png_unfilter_batch_device(None, -1, None, None, None, None, None, None, None) == ZS_STREAM_ERROR
    assert L.zs_ctx_counter(None, b"png_segments") == -1


def test_python_layer_raises_value_error_for_bad_arguments():
    from zlibstream_amd import png_unfilter_batch_device, png_unfilter_device

    class NoEngine:  # the checks come before the engine is touched
        @property
        def handle(self):
            raise AssertionError("the engine was reached")

    for row_bytes, height, bpp in ((4, 2, 0), (4, 2, 9), (0, 2, 1), (4, 0, 1), (4, 1 << 31, 4)):
        with pytest.raises(ValueError):
            png_unfilter_device(NoEngine(), 4096, row_bytes, height, bpp, 8192)
        with pytest.raises(ValueError):
            png_unfilter_batch_device(NoEngine(), [4096], [row_bytes], [height], [bpp], [8192])
    with pytest.raises(ValueError):
        png_unfilter_device(NoEngine(), 0, 4, 2, 1, 8192)
    with pytest.raises(ValueError):
        png_unfilter_batch_device(NoEngine(), [4096, 4096], [4], [2], [1], [8192])
    assert png_unfilter_batch_device(NoEngine(), [], [], [], [], []) == []


def test_schedule_model_matches_row_by_row_reconstruction():
    """tests/cpp/test_png_unfilter.cpp: the skewed lanes, the chunk-stepped waves two chunk steps apart, the wrap-around of
    segments longer than the waves, the cut rule and the bad-type scan, for bpp 1..8, row_bytes in {1, bpp-1, bpp, bpp+1, 63,
    64, 65, 1000, 4097}, heights in {1, 2, 63, 64, 65, 1023, 1024, 1025, 2049}, every single type and random types per row."""
    exe = os.path.join(ROOT, "build", "test_png_unfilter")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_png_unfilter.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-2000:]
