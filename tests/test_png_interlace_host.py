"""The interlaced PNG encode calls (zs_png_adam7_split_batch_device, zs_png_idat_interlace_batch_device,
zs_png_encode_interlace_batch_device), the parts that need no GPU: the split kernel's gather -- run on the host with the code the
kernel compiles (zs_png.h) -- against a plain restatement of PNG specification 8.2 and back through the interleave's code, once
more under the host sanitizers; the entry points at every layer; and the rejection of bad arguments before any device call."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS_STREAM_ERROR = -2
NEW = ("zs_png_adam7_split_batch_device", "zs_png_idat_interlace_batch_device", "zs_png_encode_interlace_batch_device")
SRC = os.path.join(ROOT, "tests", "cpp", "test_png_adam7_split.cpp")


def _run(exe, flags):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17"] + flags + ["-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), (r.stdout[-2000:], r.stderr[-2000:])


def test_split_model_matches_the_specification_restated():
    """tests/cpp/test_png_adam7_split.cpp: every (width, height) in 1..20 x 1..20 and (1000, 3), (257, 63), (33, 31), (65, 129) at
    every bits value, source and destination at every byte residue mod 16, the source's padding bits all ones: the kernel's
    aligned groups (4, 8 and 16 bytes) reproduce nested loops over xstart + k * xstep with sub-byte packing and zero padding
    bits, write every byte of the passes and none outside, and the interleave's code gives the rows back, padding cleared."""
    _run(os.path.join(ROOT, "build", "test_png_adam7_split"), ["-O2"])


def test_split_model_is_clean_under_the_host_sanitizers():
    """The same stand-alone program built with -fsanitize=address,undefined: its source buffers end where their allocations
    end, so a load behind a source row's last byte is an error."""
    _run(os.path.join(ROOT, "build", "test_png_adam7_split_asan"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_entry_points_resolve_at_every_layer():
    from zlibstream_amd import _native, build
    L = ctypes.CDLL(build.build_engine())
    for s in NEW:
        assert hasattr(L, s), s
        assert s in _native.SYMBOLS, s
        for f in ("include/zsgpu.h", "include/zsgpu.hpp", "dotnet/ZsGpu.cs"):
            assert s in open(os.path.join(ROOT, f)).read(), (s, f)
        fn = getattr(_native.lib(), s)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, s
    import zlibstream_amd
    for name in ("png_adam7_split_batch_device", "png_idat_interlace_batch_device", "png_encode_interlace_batch_device"):
        assert callable(getattr(zlibstream_amd, name)), name


def test_a_null_context_is_a_stream_error_whatever_else_is_passed():
    from zlibstream_amd import _native
    L = _native.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    VP, I64, I32 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_int * 1
    for w, h, bits, il in ((4, 2, 8, 1), (4, 2, 8, 0), (0, 2, 8, 1), (4, 0, 8, 1), (4, 2, 5, 1), (4, 2, 8, 3), (1 << 31, 2, 8, 1)):
        st, ln = I32(7), I64(-9)
        assert L.zs_png_adam7_split_batch_device(None, 1, VP(p), I64(w), I64(h), I32(bits), VP(p), None) == ZS_STREAM_ERROR
        assert L.zs_png_idat_interlace_batch_device(None, 1, VP(p), I64(w), I64(h), I32(bits), I32(il), I32(0), 1, VP(p), I64(64), ln, st, 6, 0, 0,
                                                    None) == ZS_STREAM_ERROR
        assert L.zs_png_encode_interlace_batch_device(None, 1, VP(p), I64(w), I64(h), I32(bits), I32(0), I32(0), I32(il), None, None, 1, 0, VP(p),
                                                      I64(64), ln, st, 6, 0, 0, None) == ZS_STREAM_ERROR
        assert st[0] == 7 and ln[0] == -9
    for n in (0, -1, 5):
        assert L.zs_png_adam7_split_batch_device(None, n, None, None, None, None, None, None) == ZS_STREAM_ERROR
        assert L.zs_png_idat_interlace_batch_device(None, n, None, None, None, None, None, None, 1, None, None, None, None, 6, 0, 0, None) == ZS_STREAM_ERROR
        assert L.zs_png_encode_interlace_batch_device(None, n, None, None, None, None, None, None, None, None, None, 1, 0, None, None, None, None, 6, 0,
                                                      0, None) == ZS_STREAM_ERROR


class NoEngine:  # the checks come before the engine is touched
    @property
    def handle(self):
        raise AssertionError("the engine was reached")


def test_split_wrapper_raises_value_error_for_bad_arguments():
    from zlibstream_amd import png_adam7_split_batch_device
    e = NoEngine()
    good = dict(pixel_ptrs=[4096], widths=[4], heights=[2], bits_per_pixel=[8], pass_ptrs=[8192])
    changes = [("widths", [0]), ("heights", [0]), ("widths", [-3]), ("heights", [1 << 31]), ("widths", [1 << 31]), ("pixel_ptrs", [0]),
               ("pixel_ptrs", [None]), ("pass_ptrs", [0]), ("widths", [4, 4]), ("pass_ptrs", []), ("heights", [])]
    changes += [("bits_per_pixel", [b]) for b in (0, 3, 5, 12, 40, 56, 72)]
    for key, value in changes:
        with pytest.raises(ValueError):
            png_adam7_split_batch_device(e, **dict(good, **{key: value}))
    # more than 2^31 - 1 pass rows in one call: an image 8 pixels wide has 15 pass rows for every 8 of its own, one 1 pixel
    # wide as many as it has rows (passes 1, 3, 5 and 7 hold its column)
    with pytest.raises(ValueError):
        png_adam7_split_batch_device(e, [4096], [8], [(1 << 31) - 8], [1], [8192])
    with pytest.raises(AssertionError):
        png_adam7_split_batch_device(e, [4096], [1], [(1 << 31) - 8], [1], [8192])
    with pytest.raises(AssertionError):
        png_adam7_split_batch_device(e, **good)
    assert png_adam7_split_batch_device(e, [], [], [], [], []) is None


def test_idat_wrapper_raises_value_error_for_bad_arguments():
    from zlibstream_amd import png_idat_interlace_batch_device
    e = NoEngine()
    good = dict(pixel_ptrs=[4096], widths=[4], heights=[2], bits_per_pixel=[8], interlace=[1], filters=[5], out_ptrs=[8192], out_caps=[4096])
    changes = [("widths", [0]), ("heights", [0]), ("heights", [1 << 31]), ("widths", [1 << 31]), ("pixel_ptrs", [0]), ("out_ptrs", [None]),
               ("interlace", [2]), ("interlace", [-1]), ("interlace", []), ("filters", [6]), ("filters", [-1]), ("filters", []), ("out_caps", []),
               ("widths", [4, 4]), ("rows_per_write", -1), ("level", 10), ("level", -2), ("strategy", 5), ("strategy", -1)]
    changes += [("bits_per_pixel", [b]) for b in (0, 3, 5, 12, 40, 56, 72)]
    for key, value in changes:
        with pytest.raises(ValueError):
            png_idat_interlace_batch_device(e, **dict(good, **{key: value}))
    # a filtered image above 2 GiB - 1 KiB, measured by the layout: 2^15 x 2^14 pixels of 4 bytes are 2 GiB and some filter bytes
    with pytest.raises(ValueError):
        png_idat_interlace_batch_device(e, **dict(good, widths=[1 << 15], heights=[1 << 14], bits_per_pixel=[32]))
    # pass rows are what is counted: five images of 8 x 2^28 have 1.25 * 2^30 rows of their own and 15 / 8 as many pass rows
    five = dict(pixel_ptrs=[4096] * 5, widths=[8] * 5, heights=[1 << 28] * 5, bits_per_pixel=[1] * 5, filters=[0] * 5, out_ptrs=[8192] * 5, out_caps=[64] * 5)
    with pytest.raises(ValueError):
        png_idat_interlace_batch_device(e, interlace=[1] * 5, **five)
    with pytest.raises(AssertionError):
        png_idat_interlace_batch_device(e, interlace=None, **five)
    with pytest.raises(AssertionError):
        png_idat_interlace_batch_device(e, **good)
    assert png_idat_interlace_batch_device(e, [], [], [], [], [], [], [], []) == []
    assert png_idat_interlace_batch_device(e, [], [], [], [], None, [], [], [], return_status=True) == (0, [], [])


def test_encode_wrapper_raises_value_error_for_bad_arguments():
    from zlibstream_amd import png_encode_interlace_batch_device
    e = NoEngine()
    good = dict(pixel_ptrs=[4096], widths=[4], heights=[2], bit_depths=[8], color_types=[2], filters=[5], out_ptrs=[8192], out_caps=[4096],
                interlace=[1])
    changes = [("widths", [0]), ("heights", [0]), ("heights", [1 << 31]), ("pixel_ptrs", [0]), ("out_ptrs", [None]), ("out_caps", [-1]),
               ("interlace", [2]), ("interlace", [-1]), ("interlace", []), ("interlace", [1, 1]), ("filters", [6]), ("filters", []),
               ("bit_depths", [4]), ("color_types", [5]), ("bit_depths", [3]), ("rows_per_write", -1),
               ("idat_chunk_bytes", -1), ("idat_chunk_bytes", 1 << 31), ("level", 10), ("strategy", 5), ("extra", [b"\x00\x00\x00\x09abcd"]),
               ("extra", [b"", b""])]
    for key, value in changes:
        with pytest.raises(ValueError):
            png_encode_interlace_batch_device(e, **dict(good, **{key: value}))
    with pytest.raises(ValueError):  # above 2 GiB - 1 KiB filtered
        png_encode_interlace_batch_device(e, **dict(good, widths=[1 << 15], heights=[1 << 14], bit_depths=[8], color_types=[6]))
    # more than 2^31 - 1 rows, pass rows counted (five images of 8 x 2^28: 1.25 * 2^30 rows of their own, 15 / 8 as many pass rows)
    five = dict(pixel_ptrs=[4096] * 5, widths=[8] * 5, heights=[1 << 28] * 5, bit_depths=[1] * 5, color_types=[0] * 5, filters=[0] * 5, out_ptrs=[8192] * 5,
                out_caps=[64] * 5)
    with pytest.raises(ValueError):
        png_encode_interlace_batch_device(e, interlace=[1] * 5, **five)
    with pytest.raises(AssertionError):
        png_encode_interlace_batch_device(e, interlace=None, **five)
    with pytest.raises(AssertionError):
        png_encode_interlace_batch_device(e, **good)
    assert png_encode_interlace_batch_device(e, [], [], [], [], [], [], [], []) == []
