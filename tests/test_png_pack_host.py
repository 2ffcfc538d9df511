"""The pack of RGBA pixels into raw PNG scanlines and the choice of a file format, the parts that need no GPU: the code the
kernel compiles (zs_png.h png_pack_group) run on the host against a per-pixel restatement of the rules
(tests/cpp/test_png_pack.cpp), zs_png_choose_format -- pure host code -- through ctypes on a table that reaches all fifteen
legal pairs, and the ValueErrors of the Python layer."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS_OK, ZS_STREAM_ERROR = 0, -2
LEGAL = [(c, d) for c, ds in ((0, (1, 2, 4, 8, 16)), (2, (8, 16)), (3, (1, 2, 4, 8)), (4, (8, 16)), (6, (8, 16))) for d in ds]


def test_group_model_matches_the_rules_restated():
    """all fifteen (color type, bit depth) pairs, both formats, widths 1..70 and 255, 256, 257, 513, heights 1 and 3, the output
    at every residue modulo 16, with and without a tRNS key, palettes of 1, 2, 16, 255 and 256 entries with duplicates and the
    entry 0,0,0,0, pixels without an entry counted; guard bytes around every output; every lookup table entry by entry."""
    exe = os.path.join(ROOT, "build", "test_png_pack")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_png_pack.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-2000:]


# ---------------------------------------------------------------- zs_png_choose_format
def S(opaque, gray, low8, sample_depth, n_colors):
    return dict(opaque=opaque, gray=gray, low8=low8, sample_depth=sample_depth, n_colors=n_colors)


# survey -> the pair the rule gives: the base where no palette is strictly narrower, the palette where it is
CHOICES = [
    (S(1, 1, 1, 1, 2), (0, 1)),      # black and white: a 1-bit palette ties with 1-bit gray, the base stays
    (S(1, 1, 1, 1, 1), (0, 1)),
    (S(1, 1, 1, 2, 4), (0, 2)),      # tie at 2 bits
    (S(1, 1, 1, 2, 2), (3, 1)),      # two of the four 2-bit grays
    (S(1, 1, 1, 4, 16), (0, 4)),     # tie at 4 bits
    (S(1, 1, 1, 4, 3), (3, 2)),
    (S(1, 1, 1, 8, 200), (0, 8)),    # tie at 8 bits
    (S(1, 1, 1, 8, 256), (0, 8)),
    (S(1, 1, 1, 8, 3), (3, 2)),      # three grays that are no multiples of 85
    (S(1, 1, 1, 8, 16), (3, 4)),
    (S(1, 1, 1, 8, 17), (0, 8)),
    (S(1, 1, 0, 16, 257), (0, 16)),
    (S(1, 0, 1, 8, 257), (2, 8)),
    (S(1, 0, 1, 8, 256), (3, 8)),
    (S(1, 0, 1, 1, 2), (3, 1)),      # red and blue, say
    (S(1, 0, 1, 1, 8), (3, 4)),
    (S(1, 0, 0, 16, 257), (2, 16)),
    (S(0, 1, 1, 8, 257), (4, 8)),
    (S(0, 1, 1, 8, 256), (3, 8)),    # 8 < 16
    (S(0, 1, 1, 1, 4), (3, 2)),
    (S(0, 1, 0, 16, 257), (4, 16)),
    (S(0, 0, 1, 8, 257), (6, 8)),
    (S(0, 0, 1, 8, 17), (3, 8)),
    (S(0, 0, 1, 8, 1), (3, 1)),
    (S(0, 0, 0, 16, 257), (6, 16)),
]


def test_the_choice_reaches_every_legal_pair_and_keeps_the_base_on_a_tie():
    from zlibstream_amd import png_choose_format
    for survey, want in CHOICES:
        assert png_choose_format(survey) == want, survey
    assert {want for _, want in CHOICES} == set(LEGAL)
    # the flags are read as truth values, and colors are not looked at
    assert png_choose_format(dict(S(7, 3, 1, 8, 3), colors=[(1, 1, 1, 255)] * 3)) == (3, 2)


def test_the_choice_refuses_what_no_survey_says():
    from zlibstream_amd import _native, png_choose_format
    L = _native.lib()
    ct, bd = ctypes.c_int(-7), ctypes.c_int(-7)
    ok = _native.PngSurvey(1, 1, 1, 8, 3)
    assert L.zs_png_choose_format(ctypes.byref(ok), ctypes.byref(ct), ctypes.byref(bd)) == ZS_OK and (ct.value, bd.value) == (3, 2)
    for bad in (_native.PngSurvey(1, 1, 1, 3, 3), _native.PngSurvey(1, 1, 1, 0, 3), _native.PngSurvey(1, 1, 1, 16, 3), _native.PngSurvey(1, 1, 0, 8, 257),
                _native.PngSurvey(1, 1, 1, 8, 0), _native.PngSurvey(1, 1, 1, 8, 258), _native.PngSurvey(1, 1, 1, 8, -1)):
        ct.value = bd.value = -7
        assert L.zs_png_choose_format(ctypes.byref(bad), ctypes.byref(ct), ctypes.byref(bd)) == ZS_STREAM_ERROR
        assert (ct.value, bd.value) == (-7, -7)
    assert L.zs_png_choose_format(None, ctypes.byref(ct), ctypes.byref(bd)) == ZS_STREAM_ERROR
    assert L.zs_png_choose_format(ctypes.byref(ok), None, ctypes.byref(bd)) == ZS_STREAM_ERROR
    assert L.zs_png_choose_format(ctypes.byref(ok), ctypes.byref(ct), None) == ZS_STREAM_ERROR
    for bad in (S(1, 1, 1, 3, 3), S(1, 1, 1, 16, 3), S(1, 1, 0, 8, 257), S(1, 1, 1, 8, 0), S(1, 1, 1, 8, 258), dict(opaque=1), None, S(1, 1, 1, "x", 3)):
        with pytest.raises(ValueError):
            png_choose_format(bad)


# ---------------------------------------------------------------- the Python layer
def test_python_layer_raises_value_error_for_bad_arguments():
    """before the library is asked: no engine and no GPU are needed to be told"""
    from zlibstream_amd import PNG_RGBA8, PNG_RGBA16, png_encode_rgba_batch_device, png_pack_batch_device, png_survey_batch_device
    ok = dict(in_ptrs=[4096], widths=[3], heights=[2], bit_depths=[8], color_types=[3], out_ptrs=[8193], plte=[b"abc"], trns=[b"\x01"], format=PNG_RGBA16)
    for change in (dict(widths=[0]), dict(heights=[1 << 31]), dict(bit_depths=[16]), dict(color_types=[5]), dict(in_ptrs=[0]), dict(out_ptrs=[0]),
                   dict(in_ptrs=[4100]), dict(plte=None), dict(plte=[b"abcd"]), dict(plte=[bytes(771)]), dict(trns=[b"\x01\x02"]), dict(format=2),
                   dict(widths=[3, 3]), dict(plte=[b"abc", b"abc"]), dict(color_types=[0], trns=[b"\x01"]), dict(color_types=[2], trns=[b"\x01\x02"])):
        with pytest.raises(ValueError):
            png_pack_batch_device(None, **dict(ok, **change))
    with pytest.raises(ValueError):
        png_pack_batch_device(None, **dict(ok, format=PNG_RGBA8, in_ptrs=[4098]))
    for args in (([4096], [3], [2, 2], PNG_RGBA8), ([0], [3], [2], PNG_RGBA8), ([4100], [3], [2], PNG_RGBA16), ([4098], [3], [2], PNG_RGBA8),
                 ([4096], [0], [2], PNG_RGBA8), ([4096], [3], [1 << 31], PNG_RGBA8), ([4096], [3], [2], 2),
                 ([4096, 4096], [1, 1], [(1 << 31) - 1, 1], PNG_RGBA8)):
        with pytest.raises(ValueError):
            png_survey_batch_device(None, *args)
    ok = dict(pixel_ptrs=[4096], widths=[3], heights=[2], filters=[5], out_ptrs=[8193], out_caps=[4096], format=PNG_RGBA16, interlace=[1], extra=[b""])
    for change in (dict(widths=[0]), dict(heights=[1 << 31]), dict(pixel_ptrs=[0]), dict(pixel_ptrs=[4100]), dict(out_ptrs=[0]), dict(out_caps=[-1]),
                   dict(filters=[6]), dict(interlace=[2]), dict(format=-1), dict(extra=[b"\x00\x00\x00\x01tEXt"]), dict(extra=[b"", b""]), dict(widths=[3, 3]),
                   dict(rows_per_write=-1), dict(idat_chunk_bytes=1 << 31), dict(level=10), dict(strategy=5), dict(widths=[1 << 30], heights=[1 << 30])):
        with pytest.raises(ValueError):
            png_encode_rgba_batch_device(None, **dict(ok, **change))
