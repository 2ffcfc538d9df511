"""Whole PNG files, the parts that need no GPU: zs_png_file_bound against a restatement, zs_png_file_info on files built here
with struct and zlib, every host-checkable way a file can be broken, the new entry points at every layer, and the rejection of
bad arguments before any device call."""
import ctypes
import os
import struct
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS_OK, ZS_STREAM_ERROR, ZS_DATA_ERROR = 0, -2, -3
SIG = b"\x89PNG\r\n\x1a\n"
NEW = ("zs_crc32_device", "zs_crc32_batch_device", "zs_png_file_bound", "zs_png_encode_batch_device", "zs_png_file_info", "zs_png_decode_files_batch")
# PNG specification table 11.1
LEGAL = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(ctype, data, crc=None):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data) if crc is None else crc)


def ihdr(w, h, depth, color, interlace=0, compression=0, filt=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color, compression, filt, interlace))


def png(w=5, h=3, depth=8, color=2, interlace=0, idat=(b"abc",), before=(), after=()):
    return SIG + ihdr(w, h, depth, color, interlace) + b"".join(before) + b"".join(chunk(b"IDAT", d) for d in idat) + b"".join(after) + chunk(b"IEND", b"")


def bound(idat_len, chunk_bytes, extra_len):
    chunks = 1 if chunk_bytes == 0 or idat_len == 0 else -(-idat_len // chunk_bytes)
    return 8 + (12 + 13) + extra_len + idat_len + 12 * chunks + 12


def test_file_bound_against_the_restatement():
    from zlibstream_amd import _native, png_file_bound
    L = _native.lib()
    for idat_len in (0, 1, 8191, 8192, 8193):
        for chunk_bytes in (0, 1, 8192, (1 << 31) - 1):
            for extra_len in (0, 12, 57):
                want = bound(idat_len, chunk_bytes, extra_len)
                assert L.zs_png_file_bound(idat_len, chunk_bytes, extra_len) == want, (idat_len, chunk_bytes, extra_len)
                assert png_file_bound(idat_len, chunk_bytes, extra_len) == want
    # what a file built here weighs
    f = png(idat=(b"x" * 10, b"y" * 10, b"z" * 3), before=(chunk(b"gAMA", b"\0\0\0\1"),))
    assert len(f) == bound(23, 10, 16)
    for bad in ((-1, 0, 0), (1, -1, 0), (1, 1 << 31, 0), (1, 0, -1), (1 << 31, 0, 0)):
        assert L.zs_png_file_bound(*bad) == -1, bad
        with pytest.raises(ValueError):
            png_file_bound(*bad)
    assert png_file_bound(1 << 31, 1 << 20, 0) == bound(1 << 31, 1 << 20, 0)  # (many chunks hold what one cannot)


def test_file_info_gives_the_fields():
    from zlibstream_amd import png_file_info
    for color, depths in LEGAL.items():
        for depth in depths:
            for interlace in (0, 1):
                for w, h in ((1, 1), (5, 3), (1000, 3)):
                    idat = (b"12345", b"", b"678")
                    f = png(w, h, depth, color, interlace, idat, before=(chunk(b"gAMA", b"\0\1\2\3"),), after=(chunk(b"tEXt", b"k\0v"),))
                    bits = depth * CHANNELS[color]
                    assert png_file_info(f) == dict(width=w, height=h, bit_depth=depth, color_type=color, interlace=interlace, bits_per_pixel=bits,
                                                    idat_bytes=8, pixel_bytes=h * ((w * bits + 7) // 8), n_idat=3), (color, depth, interlace, w, h)
    # ancillary chunks are not verified; bytes behind IEND are not the file's
    assert png_file_info(png(before=(chunk(b"gAMA", b"\0\1\2\3", crc=7),)) + b"trailing")["n_idat"] == 1
    assert png_file_info(png(w=(1 << 31) - 1, h=(1 << 31) - 1, depth=8, color=0))["pixel_bytes"] == ((1 << 31) - 1) ** 2


def broken_files():
    good = png()
    at_idat = len(SIG) + 25
    flip = lambda f, i: f[:i] + bytes([f[i] ^ 0x20]) + f[i + 1:]
    out = {
        "bad signature": flip(good, 1),
        "short signature": good[:5],
        "empty": b"",
        "truncated chunk (CRC cut)": good[:-2],
        "truncated chunk (header cut)": good[:-9],
        "truncated chunk (data cut)": good[:at_idat + 9],
        "length field past the end": good[:at_idat] + struct.pack(">I", 1000) + good[at_idat + 4:],
        "IHDR missing": SIG + chunk(b"IDAT", b"abc") + chunk(b"IEND", b""),
        "IHDR not first": SIG + chunk(b"gAMA", b"\0\1\2\3") + good[8:],
        "IHDR twice": good[:at_idat] + ihdr(5, 3, 8, 2) + good[at_idat:],
        "IHDR of 12 bytes": SIG + chunk(b"IHDR", b"\0" * 12) + good[at_idat:],
        "width 0": png(w=0),
        "height 0": png(h=0),
        "width 2^31": png(w=1 << 31),
        "interlace 2": png(interlace=2),
        "compression 1": SIG + ihdr(5, 3, 8, 2, compression=1) + good[at_idat:],
        "filter method 1": SIG + ihdr(5, 3, 8, 2, filt=1) + good[at_idat:],
        "no IDAT": SIG + ihdr(5, 3, 8, 2) + chunk(b"IEND", b""),
        "IDAT not consecutive": png(idat=(b"a",), after=(chunk(b"tEXt", b""), chunk(b"IDAT", b"b"))),
        "IEND missing": good[:-12],
        "nothing behind the signature": SIG,
        "CRC of IHDR": flip(good, len(SIG) + 8 + 2),
        "CRC of IDAT": flip(good, at_idat + 9),
        "CRC of IEND": flip(good, len(good) - 1),
        "CRC of PLTE": png(color=3, before=(chunk(b"PLTE", b"\1\2\3", crc=5),)),
    }
    for color in range(8):
        for depth in (0, 1, 2, 3, 4, 8, 16, 32):
            if depth not in LEGAL.get(color, ()):
                out["color type %d depth %d" % (color, depth)] = png(depth=depth, color=color)
    return out


def test_file_info_reports_every_host_checkable_error():
    from zlibstream_amd import ZlibStreamException, _native, png_file_info
    L = _native.lib()
    info = _native.PngInfo()
    assert L.zs_png_file_info(png(), len(png()), ctypes.byref(info)) == ZS_OK
    for name, f in broken_files().items():
        assert L.zs_png_file_info(f, len(f), ctypes.byref(info)) == ZS_DATA_ERROR, name
        with pytest.raises(ZlibStreamException):
            png_file_info(f)
    assert L.zs_png_file_info(None, 10, ctypes.byref(info)) == ZS_STREAM_ERROR
    assert L.zs_png_file_info(png(), 10, None) == ZS_STREAM_ERROR
    assert L.zs_png_file_info(png(), -1, ctypes.byref(info)) == ZS_STREAM_ERROR


def test_entry_points_resolve_at_every_layer():
    from zlibstream_amd import _native, build
    L = ctypes.CDLL(build.build_engine())
    for s in NEW:
        assert hasattr(L, s), s
        assert s in _native.SYMBOLS, s
        for f in ("include/zsgpu.h", "include/zsgpu.hpp", "dotnet/ZsGpu.cs"):
            assert s in open(os.path.join(ROOT, f)).read(), (s, f)
    import zlibstream_amd
    for name in ("crc32_device", "crc32_batch_device", "png_file_bound", "png_encode_batch_device", "png_file_info", "png_decode_files_batch"):
        assert callable(getattr(zlibstream_amd, name)), name


def test_a_null_context_is_a_stream_error_whatever_else_is_passed():
    from zlibstream_amd import _native
    L = _native.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    VP, I64, I32, U32 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_int * 1, ctypes.c_uint32 * 1
    st, out_len, crc = I32(7), I64(9), U32(11)
    assert L.zs_crc32_device(None, p, 4, 0, crc, None) == ZS_STREAM_ERROR
    assert L.zs_crc32_batch_device(None, 1, VP(p), I64(4), None, crc, None) == ZS_STREAM_ERROR
    assert L.zs_png_encode_batch_device(None, 1, VP(p), I64(2), I64(2), I32(8), I32(0), I32(0), None, None, 1, 0, VP(p), I64(64), out_len, st, 6, 0, 0,
                                        None) == ZS_STREAM_ERROR
    f = png()
    fb = ctypes.create_string_buffer(f, len(f))
    assert L.zs_png_decode_files_batch(None, 1, VP(ctypes.addressof(fb)), I64(len(f)), VP(p), I64(64), None, st, None) == ZS_STREAM_ERROR
    for n in (0, -1, 5):
        assert L.zs_crc32_batch_device(None, n, None, None, None, None, None) == ZS_STREAM_ERROR
        assert L.zs_png_encode_batch_device(None, n, None, None, None, None, None, None, None, None, 0, 0, None, None, None, None, 6, 0, 0, None) == ZS_STREAM_ERROR
        assert L.zs_png_decode_files_batch(None, n, None, None, None, None, None, None, None) == ZS_STREAM_ERROR
    assert (st[0], out_len[0], crc[0]) == (7, 9, 11)


class NoEngine:  # the checks come before the engine is touched
    @property
    def handle(self):
        raise AssertionError("the engine was reached")


def test_python_layer_raises_value_error_for_bad_arguments():
    from zlibstream_amd import crc32_batch_device, crc32_device, png_decode_files_batch, png_encode_batch_device
    e = NoEngine()
    good = dict(pixel_ptrs=[4096], widths=[4], heights=[2], bit_depths=[8], color_types=[2], filters=[5], out_ptrs=[8192], out_caps=[1000])
    changes = [("widths", [0]), ("heights", [0]), ("widths", [1 << 31]), ("heights", [-1]), ("pixel_ptrs", [0]), ("out_ptrs", [None]), ("filters", [6]),
               ("filters", [-1]), ("out_caps", [-1]), ("widths", [4, 4]), ("out_caps", []), ("bit_depths", [4]), ("bit_depths", [32]), ("color_types", [1]),
               ("color_types", [5]), ("color_types", [7]), ("heights", [1 << 30])]
    for key, value in changes:
        with pytest.raises(ValueError):
            png_encode_batch_device(e, **dict(good, **{key: value}))
    for kw in (dict(rows_per_write=-1), dict(idat_chunk_bytes=-1), dict(idat_chunk_bytes=1 << 31), dict(level=10), dict(strategy=5), dict(extra=[b"abc"]),
               dict(extra=[struct.pack(">I", 5) + b"tEXt" + b"ab" + b"\0\0\0\0"]), dict(extra=[b"", b""])):
        with pytest.raises(ValueError):
            png_encode_batch_device(e, **dict(good, **kw))
    with pytest.raises(AssertionError):
        png_encode_batch_device(e, extra=[chunk(b"tEXt", b"ab") + chunk(b"gAMA", b"")], **good)
    assert png_encode_batch_device(e, [], [], [], [], [], [], [], []) == []
    for a in (([b"x"], [0], [10]), ([b"x"], [4096], [-1]), ([b"x"], [4096, 4096], [10, 10]), ([b"x"], [4096], [])):
        with pytest.raises(ValueError):
            png_decode_files_batch(e, *a)
    assert png_decode_files_batch(e, [], [], []) == ([], [])
    for a in ((4096, -1), (4096, 1 << 31), (0, 1)):
        with pytest.raises(ValueError):
            crc32_device(e, *a)
        with pytest.raises(ValueError):
            crc32_batch_device(e, [a[0]], [a[1]])
    assert crc32_batch_device(e, [], []) == []
