"""The expansion of raw PNG scanlines to RGBA, the parts that need no GPU: the code the kernel compiles (zs_png.h
png_expand_group) run on the host against a per-pixel restatement of the rules (tests/cpp/test_png_expand.cpp), and
zs_png_file_colors -- pure host code -- on hand-built files through ctypes."""
import ctypes
import os
import struct
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS_OK, ZS_STREAM_ERROR, ZS_DATA_ERROR = 0, -2, -3
SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def test_group_model_matches_the_rules_restated():
    """all fifteen (color type, bit depth) pairs, both formats, widths 1..70 and 255, 256, 257, 513, heights 1 and 3, the output
    at every legal residue modulo 16, with and without tRNS (keys that match some pixels, and differ from others in one bit),
    palettes of 1, 2, 16, 255 and 256 entries with indexes beyond them; guard bytes around every output."""
    exe = os.path.join(ROOT, "build", "test_png_expand")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_png_expand.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-2000:]


# ---------------------------------------------------------------- zs_png_file_colors
def chunk(ctype, data, crc=None):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data) if crc is None else crc)


def flipped(ctype, data):
    return chunk(ctype, data, crc=zlib.crc32(ctype + data) ^ 0x10)


def png(color, depth, before=(), after=(), w=2, h=2):
    """a whole 2 x 2 file: `before` between IHDR and IDAT, `after` between IDAT and IEND"""
    rb = (w * depth * CHANNELS[color] + 7) // 8
    return (SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color, 0, 0, 0)) + b"".join(before) +
            chunk(b"IDAT", zlib.compress(bytes(h * (rb + 1)))) + b"".join(after) + chunk(b"IEND", b""))


def colors(f):
    """-> (rc, plte bytes, trns bytes) straight from the C entry point"""
    from zlibstream_amd import _native
    plte, trns = (ctypes.c_uint8 * 768)(), (ctypes.c_uint8 * 256)()
    n_plte, n_trns = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = _native.lib().zs_png_file_colors(f, len(f), plte, ctypes.byref(n_plte), trns, ctypes.byref(n_trns))
    if rc != ZS_OK:
        return rc, None, None
    return rc, bytes(plte[:3 * n_plte.value]), bytes(trns[:n_trns.value])


PLTE5 = bytes(range(10, 25))
PLTE256 = bytes((7 * i + 3) & 255 for i in range(768))


def test_plte_and_trns_come_back_byte_for_byte():
    gama = chunk(b"gAMA", struct.pack(">I", 45455))
    assert colors(png(0, 8, [gama, chunk(b"tRNS", b"\x12\x34")])) == (ZS_OK, b"", b"\x12\x34")
    assert colors(png(0, 16)) == (ZS_OK, b"", b"")
    assert colors(png(2, 8, [chunk(b"tRNS", b"\x00\x01\xff\x02\x00\x03")])) == (ZS_OK, b"", b"\x00\x01\xff\x02\x00\x03")
    # (a PLTE of a truecolor file is a suggested palette: returned, and of no use to the expansion)
    assert colors(png(2, 16, [chunk(b"PLTE", PLTE5), chunk(b"tRNS", bytes(6))])) == (ZS_OK, PLTE5, bytes(6))
    assert colors(png(3, 4, [chunk(b"PLTE", PLTE5)])) == (ZS_OK, PLTE5, b"")
    assert colors(png(3, 4, [chunk(b"PLTE", PLTE5), gama, chunk(b"tRNS", b"\x00\x80\xff")])) == (ZS_OK, PLTE5, b"\x00\x80\xff")
    assert colors(png(3, 8, [chunk(b"PLTE", PLTE256), chunk(b"tRNS", bytes(range(256)))])) == (ZS_OK, PLTE256, bytes(range(256)))
    assert colors(png(3, 1, [chunk(b"PLTE", b"abc"), chunk(b"tRNS", b"\x07")])) == (ZS_OK, b"abc", b"\x07")


REJECTED = {
    "PLTE no multiple of 3": png(3, 8, [chunk(b"PLTE", bytes(16))]),
    "PLTE empty": png(3, 8, [chunk(b"PLTE", b"")]),
    "PLTE of 257 entries": png(3, 8, [chunk(b"PLTE", bytes(771))]),
    "PLTE of a truecolor file no multiple of 3": png(2, 8, [chunk(b"PLTE", bytes(4))]),
    "a second PLTE": png(3, 8, [chunk(b"PLTE", PLTE5), chunk(b"PLTE", PLTE5)]),
    "a second tRNS": png(0, 8, [chunk(b"tRNS", bytes(2)), chunk(b"tRNS", bytes(2))]),
    "PLTE behind IDAT": png(2, 8, after=[chunk(b"PLTE", PLTE5)]),
    "the only PLTE of a palette file behind IDAT": png(3, 8, after=[chunk(b"PLTE", PLTE5)]),
    "tRNS behind IDAT": png(0, 8, after=[chunk(b"tRNS", bytes(2))]),
    "tRNS of a palette file behind IDAT": png(3, 8, [chunk(b"PLTE", PLTE5)], after=[chunk(b"tRNS", bytes(2))]),
    "palette file without PLTE": png(3, 2),
    "tRNS in front of PLTE": png(3, 8, [chunk(b"tRNS", bytes(2)), chunk(b"PLTE", PLTE5)]),
    "tRNS of 3 bytes at type 0": png(0, 8, [chunk(b"tRNS", bytes(3))]),
    "tRNS of 6 bytes at type 0": png(0, 16, [chunk(b"tRNS", bytes(6))]),
    "tRNS of 2 bytes at type 2": png(2, 8, [chunk(b"tRNS", bytes(2))]),
    "tRNS of 7 bytes at type 2": png(2, 16, [chunk(b"tRNS", bytes(7))]),
    "tRNS longer than PLTE": png(3, 8, [chunk(b"PLTE", PLTE5), chunk(b"tRNS", bytes(6))]),
    "tRNS empty at type 3": png(3, 8, [chunk(b"PLTE", PLTE5), chunk(b"tRNS", b"")]),
    "tRNS empty at type 0": png(0, 8, [chunk(b"tRNS", b"")]),
    "tRNS with a wrong CRC at type 0": png(0, 8, [flipped(b"tRNS", bytes(2))]),
    "tRNS with a wrong CRC at type 3": png(3, 8, [chunk(b"PLTE", PLTE5), flipped(b"tRNS", bytes(3))]),
    "what zs_png_file_info rejects: a wrong PLTE CRC": png(3, 8, [flipped(b"PLTE", PLTE5)]),
    "what zs_png_file_info rejects: no IEND": png(0, 8)[:-12],
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_every_rejection_has_its_file(case):
    from zlibstream_amd import ZlibStreamException, png_file_colors
    assert colors(REJECTED[case])[0] == ZS_DATA_ERROR
    with pytest.raises(ZlibStreamException):
        png_file_colors(REJECTED[case])


def test_chunks_without_a_meaning_at_their_color_type_are_ignored():
    from zlibstream_amd import png_file_colors
    for color in (4, 6):  # a tRNS of any length, anywhere, twice, even one that is not whole by its CRC
        for d in (8, 16):
            assert colors(png(color, d, [chunk(b"tRNS", bytes(5)), flipped(b"tRNS", bytes(2))], after=[chunk(b"tRNS", b"")])) == (ZS_OK, b"", b"")
    assert colors(png(6, 8, [chunk(b"PLTE", PLTE5), chunk(b"tRNS", bytes(1))])) == (ZS_OK, PLTE5, b"")
    for color in (0, 4):  # a PLTE of any length, anywhere, twice (its CRC is a critical chunk's: zs_png_file_info's walk checks it)
        assert colors(png(color, 8, [chunk(b"PLTE", bytes(4)), chunk(b"PLTE", PLTE5)], after=[chunk(b"PLTE", b"")])) == (ZS_OK, b"", b"")
    assert colors(png(0, 8, [chunk(b"PLTE", PLTE5), chunk(b"tRNS", b"\x00\x09")])) == (ZS_OK, b"", b"\x00\x09")
    assert png_file_colors(png(4, 8, [chunk(b"PLTE", PLTE5), chunk(b"tRNS", bytes(9))])) == (b"", b"")


def test_an_ancillary_chunk_is_still_not_verified_and_a_trns_is():
    from zlibstream_amd import png_file_colors, png_file_info
    gama = flipped(b"gAMA", struct.pack(">I", 45455))
    assert colors(png(0, 8, [gama, chunk(b"tRNS", b"\x00\x05")])) == (ZS_OK, b"", b"\x00\x05")
    assert colors(png(3, 8, [gama, chunk(b"PLTE", PLTE5), gama, chunk(b"tRNS", b"\x05")], after=[gama])) == (ZS_OK, PLTE5, b"\x05")
    bad = png(2, 8, [gama, flipped(b"tRNS", bytes(6))])
    assert colors(bad)[0] == ZS_DATA_ERROR
    assert png_file_info(bad)["color_type"] == 2  # (the walk that interprets nothing still takes the file)
    assert png_file_colors(png(2, 8, [gama, chunk(b"tRNS", bytes(6))])) == (b"", bytes(6))


def test_null_pointers_and_a_negative_length_are_stream_errors():
    from zlibstream_amd import _native
    L = _native.lib()
    f = png(0, 8)
    plte, trns = (ctypes.c_uint8 * 768)(), (ctypes.c_uint8 * 256)()
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    good = [f, len(f), plte, ctypes.byref(a), trns, ctypes.byref(b)]
    assert L.zs_png_file_colors(*good) == ZS_OK
    for i in (0, 2, 3, 4, 5):
        args = list(good)
        args[i] = None
        assert L.zs_png_file_colors(*args) == ZS_STREAM_ERROR, i
    assert L.zs_png_file_colors(f, -1, plte, ctypes.byref(a), trns, ctypes.byref(b)) == ZS_STREAM_ERROR


def test_python_layer_raises_value_error_for_bad_arguments():
    """before the library is asked: no engine and no GPU are needed to be told"""
    from zlibstream_amd import PNG_RGBA8, PNG_RGBA16, png_decode_files_rgba_batch, png_expand_batch_device
    ok = dict(in_ptrs=[4096], widths=[3], heights=[2], bit_depths=[8], color_types=[3], out_ptrs=[8192], plte=[b"abc"], trns=[b"\x01"], format=PNG_RGBA16)
    for change in (dict(widths=[0]), dict(heights=[1 << 31]), dict(bit_depths=[16]), dict(color_types=[5]), dict(in_ptrs=[0]), dict(out_ptrs=[0]),
                   dict(out_ptrs=[8196]), dict(plte=None), dict(plte=[b"abcd"]), dict(plte=[bytes(771)]), dict(trns=[b"\x01\x02"]), dict(format=2),
                   dict(widths=[3, 3]), dict(plte=[b"abc", b"abc"]), dict(color_types=[0], trns=[b"\x01"]), dict(color_types=[2], trns=[b"\x01\x02"])):
        with pytest.raises(ValueError):
            png_expand_batch_device(None, **dict(ok, **change))
    with pytest.raises(ValueError):
        png_expand_batch_device(None, **dict(ok, format=PNG_RGBA8, out_ptrs=[8194]))
    f = png(0, 8)
    for args in (([f], [4096, 8192], [64], PNG_RGBA8), ([f], [0], [64], PNG_RGBA8), ([f], [4100], [64], PNG_RGBA16), ([f], [4098], [64], PNG_RGBA8),
                 ([f], [4096], [-1], PNG_RGBA8), ([f], [4096], [64], 3)):
        with pytest.raises(ValueError):
            png_decode_files_rgba_batch(None, *args)
