"""The animated PNG encoder, the parts that need no GPU: the code the frame diff (KD), the crop and the closing of an fdAT
chunk compile (zs_png.h png_diff_*, png_crop_group, zs_crc32.h png_close_chunk) run on the host against restatements of
their rules (tests/cpp/test_png_diff.cpp), and zs_png_anim_bound, which is pure host code."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGBA8, RGBA16 = 0, 1


def test_diff_crop_and_chunk_closing_match_the_rules_restated():
    """The diff driven wave by wave, lane by lane, the ballot as a 64-bit mask, one record per wave and frame, the records
    folded in another order than the device's -- against the bounding box of the differing pixels, pixel by pixel: canvases of
    1x1, 1x5, 3x1, 5x3, 261x2, 257x3 and 129x3 in both formats; no change, one pixel at each corner and on each edge, on both
    sides of a group's (3 | 4, 1 | 2) and a stretch's (255 | 256, 127 | 128) boundary, the alpha byte only, the low byte of a
    sample only, a colour under alpha 0, two opposite corners; A, B, A; 1, 2, 3 and 9 frames; every legal residue of the
    canvases modulo 16.  The crop on rectangles touching every edge, of width 1, at every pair of source and destination
    residues, with guard bytes.  The closing of a chunk with and without a prefix against struct.pack + zlib.crc32 bytes."""
    exe = os.path.join(ROOT, "build", "test_png_diff")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_png_diff.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-2000:]


def test_the_chunk_constants_of_the_host_test_are_the_format_s():
    """the bytes written into tests/cpp/test_png_diff.cpp are what png_anim_ref.chunk / fdat give"""
    from png_anim_ref import chunk, fdat
    text = open(os.path.join(ROOT, "tests", "cpp", "test_png_diff.cpp")).read()
    for b in (chunk(b"IDAT", b"hello"), fdat(7, b"hello"), chunk(b"IDAT", b""), fdat(0x01020304, b"")):
        assert ", ".join("0x%02X" % x for x in b) in text
    assert fdat(65536, bytes(range(40)))[-4:] == bytes((0xB9, 0x5F, 0xF4, 0x48)) and fdat(65536, bytes(range(40)))[:12] == bytes.fromhex("0000002C6664415400010000")


def test_anim_bound_refuses_bad_arguments():
    from zlibstream_amd import png_anim_bound
    assert png_anim_bound(8, 8, 3) > 0
    for args in ((0, 8, 3), (8, 0, 3), (1 << 31, 8, 3), (8, 1 << 31, 3), (8, 8, 0), (8, 8, -1), (8, 8, 3, 2), (8, 8, 3, -1), (8, 8, 3, RGBA8, 2), (8, 8, 3, RGBA8, -1),
                 (8, 8, 3, RGBA8, 0, -1), (8, 8, 3, RGBA8, 0, 1 << 31), (8, 8, 3, RGBA8, 0, 0, -1), (1 << 16, 1 << 16, 2), (1 << 15, 1 << 14, 2, RGBA16), (8, 8, 1 << 40)):
        assert png_anim_bound(*args) == -1, args


def test_anim_bound_is_monotone_and_covers_the_still_bound():
    from zlibstream_amd import deflate_bound, png_anim_bound, png_file_bound, png_idat_layout
    base = dict(width=33, height=21, n_frames=4, format=RGBA8, interlace=0, idat_chunk_bytes=64, extra_len=24)
    b0 = png_anim_bound(**base)
    for key, more in (("width", 34), ("height", 22), ("n_frames", 5), ("format", RGBA16), ("interlace", 1), ("extra_len", 25)):
        assert png_anim_bound(**dict(base, **{key: more})) >= b0, key
    # more room per chunk is fewer chunks; 0 is one chunk per frame, the fewest
    by_chunk = [png_anim_bound(**dict(base, idat_chunk_bytes=c)) for c in (1, 2, 7, 64, 65, 4096, 1 << 20, 0)]
    assert by_chunk == sorted(by_chunk, reverse=True) and by_chunk[0] > by_chunk[-1]
    widths = [png_anim_bound(**dict(base, width=w)) for w in range(1, 70)]
    assert widths == sorted(widths)
    frames = [png_anim_bound(**dict(base, n_frames=f)) for f in range(1, 12)]
    assert all(b > a for a, b in zip(frames, frames[1:]))
    for w, h, fmt, il, cb, xl in ((1, 1, RGBA8, 0, 0, 0), (33, 21, RGBA8, 1, 7, 12), (40, 24, RGBA16, 0, 0, 100), (257, 3, RGBA16, 1, 1000, 0)):
        z = deflate_bound(png_idat_layout(w, h, 64 if fmt == RGBA16 else 32, il)[0])
        assert png_anim_bound(w, h, 1, fmt, il, cb, xl) >= png_file_bound(z, cb, xl + 1048)
        # what the parts add up to: 12 per IDAT, 16 per fdAT, 38 per fcTL, 20 for acTL, 1048 for PLTE + tRNS
        chunks = 1 if cb == 0 else -(-z // cb)
        assert png_anim_bound(w, h, 3, fmt, il, cb, xl) == 8 + 25 + xl + 1048 + 20 + 38 + z + 12 * chunks + 2 * (38 + z + 16 * chunks) + 12


def test_the_wrappers_check_their_arguments_without_a_gpu():
    from zlibstream_amd import png_crop_batch_device, png_diff_batch_device, png_encode_anim_batch_device

    class NoEngine:
        handle = None

    e = NoEngine()
    with pytest.raises(ValueError):
        png_diff_batch_device(e, [4096], [2], [8], [8], format=2)
    with pytest.raises(ValueError):
        png_diff_batch_device(e, [4098], [2], [8], [8])
    with pytest.raises(ValueError):
        png_diff_batch_device(e, [4100], [2], [8], [8], format=RGBA16)
    with pytest.raises(ValueError):
        png_diff_batch_device(e, [4096], [0], [8], [8])
    with pytest.raises(ValueError):
        png_crop_batch_device(e, [4096], [8], [4], [0], [5], [2], [8192])
    with pytest.raises(ValueError):
        png_crop_batch_device(e, [4096], [8], [0], [0], [5], [2], [8192], pixel_bytes=3)
    with pytest.raises(ValueError):
        png_encode_anim_batch_device(e, [4096], [2], [8], [8], [0], [8192], [4096], delays=[[(1, 10), (65536, 10)]])
    with pytest.raises(ValueError):
        png_encode_anim_batch_device(e, [4096], [2], [8], [8], [0], [8192], [4096], n_plays=[-1])
    with pytest.raises(ValueError):
        png_encode_anim_batch_device(e, [4096], [2], [8], [8], [0], [8192], [4096], delays=[[(1, 10)]])
    assert png_diff_batch_device(e, [], [], [], []) == [] and png_encode_anim_batch_device(e, [], [], [], [], [], [], []) == ([], [], [], [])
