"""The PNG decode call (zs_png_decode_batch_device), the Adam7 interleave (zs_png_adam7_merge_batch_device) and the geometry
they share (zs_png_idat_layout), the parts that need no GPU: the layout against tables written out by hand, the entry points at
every layer, the rejection of bad arguments before any device call, and the interleave kernel's gather -- run on the host with
the code the kernel compiles (zs_png.h) -- against a plain restatement of PNG specification 8.2."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS_STREAM_ERROR = -2
BITS = (1, 2, 4, 8, 16, 24, 32, 48, 64)
NEW = ("zs_png_idat_layout", "zs_png_adam7_merge_batch_device", "zs_png_decode_batch_device")

# (width, height, bits) -> (inflated bytes, row_bytes[7], rows[7]), from the table of PNG specification 8.2 by hand:
# pass width = ceil((w - xstart) / xstep), height likewise, an empty pass absent; a row is ceil(width * bits / 8) bytes and
# one filter byte
BY_HAND = {
    (4, 4, 1): (14, [1, 0, 0, 1, 1, 1, 1], [1, 0, 0, 1, 1, 2, 2]),
    (4, 4, 24): (55, [3, 0, 0, 3, 6, 6, 12], [1, 0, 0, 1, 1, 2, 2]),
    (5, 3, 1): (14, [1, 1, 0, 1, 1, 1, 1], [1, 1, 0, 1, 1, 2, 1]),
    (5, 3, 24): (52, [3, 3, 0, 3, 9, 6, 15], [1, 1, 0, 1, 1, 2, 1]),
    (8, 8, 1): (30, [1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 2, 2, 4, 4]),
    (8, 8, 24): (207, [3, 3, 6, 6, 12, 12, 24], [1, 1, 1, 2, 2, 4, 4]),
    (9, 9, 1): (42, [1, 1, 1, 1, 1, 1, 2], [2, 2, 1, 3, 2, 5, 4]),
    (9, 9, 24): (262, [6, 3, 9, 6, 15, 12, 27], [2, 2, 1, 3, 2, 5, 4]),
}


def _c_layout(L, w, h, bits, interlace):
    rb, rows = (ctypes.c_int64 * 7)(*[-7] * 7), (ctypes.c_int64 * 7)(*[-7] * 7)
    return L.zs_png_idat_layout(w, h, bits, interlace, rb, rows), list(rb), list(rows)


def test_idat_layout_matches_the_tables_written_by_hand():
    from zlibstream_amd import _native, png_idat_layout
    L = _native.lib()
    assert _c_layout(L, 1, 1, 8, 1) == (2, [1, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0])  # pass 1 only
    assert png_idat_layout(1, 1, 8, 1) == (2, [1, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0])
    for (w, h, bits), want in BY_HAND.items():
        assert _c_layout(L, w, h, bits, 1) == want, (w, h, bits)
        assert png_idat_layout(w, h, bits, 1) == want, (w, h, bits)
    # not interlaced: entry 0 is the image
    assert _c_layout(L, 9, 5, 1, 0) == (5 * 3, [2, 0, 0, 0, 0, 0, 0], [5, 0, 0, 0, 0, 0, 0])
    assert png_idat_layout(1000, 3, 48, 0) == (3 * 6001, [6000, 0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0])
    assert L.zs_png_idat_layout(9, 9, 24, 1, None, None) == 262  # (either array may be left out)
    # the passes hold the image's pixels whatever its shape
    for bits in BITS:
        for w, h in ((1, 9), (9, 1), (2, 2), (3, 5), (13, 17), (257, 63), (1000, 3)):
            total, rb, rows = png_idat_layout(w, h, bits, 1)
            assert total == sum(r * (b + 1) for b, r in zip(rb, rows))
            assert all((b == 0) == (r == 0) for b, r in zip(rb, rows))
            if bits >= 8:
                assert sum(b * r for b, r in zip(rb, rows)) == w * h * bits // 8


def test_idat_layout_rejects_bad_arguments():
    from zlibstream_amd import _native, png_idat_layout
    L = _native.lib()
    bad = [(0, 4, 8, 1), (4, 0, 8, 1), (-1, 4, 8, 0), (4, -1, 8, 0), (1 << 31, 4, 8, 1), (4, 1 << 31, 8, 0), (4, 4, 8, 2), (4, 4, 8, -1)]
    bad += [(4, 4, b, 1) for b in (0, -8, 3, 5, 7, 12, 40, 56, 72, 128)]
    for a in bad:
        assert _c_layout(L, *a)[0] == -1, a
        with pytest.raises(ValueError):
            png_idat_layout(*a)


def test_entry_points_resolve_at_every_layer():
    from zlibstream_amd import _native, build
    L = ctypes.CDLL(build.build_engine())
    for s in NEW:
        assert hasattr(L, s), s
        assert s in _native.SYMBOLS, s
        for f in ("include/zsgpu.h", "include/zsgpu.hpp", "dotnet/ZsGpu.cs"):
            assert s in open(os.path.join(ROOT, f)).read(), (s, f)
    import zlibstream_amd
    for name in ("png_idat_layout", "png_adam7_merge_batch_device", "png_decode_batch_device"):
        assert callable(getattr(zlibstream_amd, name)), name


def test_a_null_context_is_a_stream_error_whatever_else_is_passed():
    from zlibstream_amd import _native
    L = _native.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    VP, I64, I32 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_int * 1
    for w, h, bits, il in ((4, 2, 8, 1), (4, 2, 8, 0), (0, 2, 8, 1), (4, 0, 8, 1), (4, 2, 5, 1), (4, 2, 8, 3), (1 << 31, 2, 8, 1)):
        st = I32(7)
        assert L.zs_png_decode_batch_device(None, 1, VP(p), I64(16), I64(w), I64(h), I32(bits), I32(il), VP(p), st, None) == ZS_STREAM_ERROR
        assert st[0] == 7
        assert L.zs_png_adam7_merge_batch_device(None, 1, VP(p), I64(w), I64(h), I32(bits), VP(p), None) == ZS_STREAM_ERROR
    for n in (0, -1, 5):
        assert L.zs_png_decode_batch_device(None, n, None, None, None, None, None, None, None, None, None) == ZS_STREAM_ERROR
        assert L.zs_png_adam7_merge_batch_device(None, n, None, None, None, None, None, None) == ZS_STREAM_ERROR


class NoEngine:  # the checks come before the engine is touched
    @property
    def handle(self):
        raise AssertionError("the engine was reached")


def test_python_layer_raises_value_error_for_bad_arguments():
    from zlibstream_amd import png_adam7_merge_batch_device, png_decode_batch_device
    e = NoEngine()
    good = dict(idat_ptrs=[4096], idat_lens=[20], widths=[4], heights=[2], bits_per_pixel=[8], interlace=[1], out_ptrs=[8192])
    changes = [("widths", [0]), ("heights", [0]), ("widths", [-3]), ("heights", [1 << 31]), ("widths", [1 << 31]),
               ("idat_ptrs", [0]), ("idat_ptrs", [None]), ("out_ptrs", [0]), ("interlace", [2]), ("interlace", [-1]),
               ("idat_lens", [-1]), ("idat_lens", [1 << 31]), ("widths", [4, 4]), ("idat_lens", []), ("out_ptrs", [])]
    changes += [("bits_per_pixel", [b]) for b in (0, 3, 5, 12, 40, 56, 72)]
    for key, value in changes:
        with pytest.raises(ValueError):
            png_decode_batch_device(e, **dict(good, **{key: value}))
    for key, value in changes:
        if key in ("interlace", "idat_lens"):
            continue
        a = dict(good, **{key: value})
        with pytest.raises(ValueError):
            png_adam7_merge_batch_device(e, a["idat_ptrs"], a["widths"], a["heights"], a["bits_per_pixel"], a["out_ptrs"])
    # more than 2^31 - 1 rows in one call, pass rows counted: three images of 2^30 rows are above it either way ...
    big = dict(idat_ptrs=[4096] * 3, idat_lens=[20] * 3, widths=[1] * 3, heights=[1 << 30] * 3, bits_per_pixel=[1] * 3, out_ptrs=[8192] * 3)
    for il in (0, 1):
        with pytest.raises(ValueError):
            png_decode_batch_device(e, interlace=[il] * 3, **big)
    with pytest.raises(ValueError):
        png_adam7_merge_batch_device(e, big["idat_ptrs"], big["widths"], big["heights"], big["bits_per_pixel"], big["out_ptrs"])
    # ... and one interlaced image 8 pixels wide has 15 pass rows for every 8 of its own: 2^31 - 8 rows are too many
    # interlaced and pass as they are (the engine is reached)
    wide = dict(idat_ptrs=[4096], idat_lens=[20], widths=[8], heights=[(1 << 31) - 8], bits_per_pixel=[1], out_ptrs=[8192])
    with pytest.raises(ValueError):
        png_decode_batch_device(e, interlace=[1], **wide)
    with pytest.raises(AssertionError):
        png_decode_batch_device(e, interlace=[0], **wide)
    assert png_decode_batch_device(e, [], [], [], [], [], [], []) == []
    assert png_adam7_merge_batch_device(e, [], [], [], [], []) is None


def test_gather_model_matches_the_specification_restated():
    """tests/cpp/test_png_adam7.cpp: every (width, height) in 1..20 x 1..20 and (1000, 3), (257, 63) at every bit depth -- the
    pass sizes sum to the image, the inverse map is a bijection onto the present passes' pixels, and the kernel's aligned
    groups (4, 8 and 16 bytes, the row at every alignment) reproduce nested loops over xstart + k * xstep with sub-byte
    packing and zero padding bits, touching nothing outside the image."""
    exe = os.path.join(ROOT, "build", "test_png_adam7")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_png_adam7.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-2000:]
