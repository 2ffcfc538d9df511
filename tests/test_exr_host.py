"""The host side of the OpenEXR calls, no GPU: the container rules of zlibstream_amd/csrc/zs_exr.h and the predictor kernels'
per-lane step run by tests/cpp/test_exr_walk.cpp under the address and undefined-behaviour sanitizers, exr_file_info against
tests/exr_cases.py on every legal shape, every error class beside its nearest legal file, exr_bound, the argument checks of
the device calls that are decided before any device work, and the model reading the builder's files back."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import exr_cases as xc
from zlibstream_amd import ZlibStreamException, _native, exr_bound, exr_decode_files, exr_encode, exr_file_info, exr_predict, exr_unpredict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS_STREAM_ERROR, ZS_DATA_ERROR, ZS_BUF_ERROR = -2, -3, -5
RGBA = [("A", xc.HALF), ("B", xc.HALF), ("G", xc.HALF), ("R", xc.HALF)]
MIXED = [("A", xc.HALF), ("B", xc.HALF), ("G", xc.HALF), ("R", xc.HALF), ("Z", xc.FLOAT), ("id", xc.UINT)]


def code_of(data):
    """zs_exr_file_info's return code and the info as far as it got."""
    data = bytes(data)
    info = _native.ExrInfo()
    return _native.lib().zs_exr_file_info(data, len(data), info, None, 0, None, 0), info


def small_files():
    return [xc.simple(9, 37, MIXED, seed=2, x_min=-4, y_min=-30)[0], xc.simple(37, 53, RGBA, seed=3, tile=(16, 16), junk=3)[0],
            xc.simple(5, 7, RGBA, seed=4, compression=2, line_order=1)[0], xc.simple(3, 4, xc.RG, seed=5, compression=0, long_names=True)[0]]


def test_shared_exr_rules_on_the_host_under_sanitizers():
    """tests/cpp/test_exr_walk.cpp, a stand-alone program built with -fsanitize=address,undefined: the walk on every prefix of
    four built files, each in a heap block of exactly its length; the writer's head read back; the kernels' per-lane step
    over a model of the wave against a scalar loop."""
    build = os.path.join(ROOT, "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_exr_walk")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_exr_walk.cpp")], check=True)
    paths = []
    for k, data in enumerate(small_files()):
        paths.append(os.path.join(build, "test_exr_walk_%d.exr" % k))
        with open(paths[-1], "wb") as f:
            f.write(data)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), (r.stdout[-2000:], r.stderr[-3000:])


def test_the_worked_example_and_the_model():
    assert xc.predict(bytes([1, 2, 3, 4, 5])) == bytes([0x01, 0x82, 0x82, 0x7D, 0x82])
    assert xc.unpredict(bytes([0x01, 0x82, 0x82, 0x7D, 0x82])) == bytes([1, 2, 3, 4, 5])
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 16, 17, 1000, 1001):
        raw = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        t = xc.predict(raw)
        # the rule as a loop
        h = (n + 1) // 2
        split = raw[0::2] + raw[1::2]
        assert t == bytes([split[0]] + [(split[i] - split[i - 1] + 128) & 255 for i in range(1, n)]) and len(raw[0::2]) == h
        assert xc.unpredict(t) == raw


SHAPES = [dict(), dict(compression=2), dict(compression=0), dict(x_min=-7, y_min=-40), dict(line_order=1), dict(tile=(16, 16)), dict(tile=(32, 8), line_order=2),
          dict(tile=(16, 16), line_order=1), dict(raw_chunks=(1,)), dict(junk=5), dict(body_order=(2, 0, 3, 1)), dict(long_names=True), dict(display=False)]


@pytest.mark.parametrize("kw", SHAPES, ids=[",".join(sorted(k)) or "plain" for k in SHAPES])
def test_file_info_and_the_model_on_every_legal_shape(kw):
    W, H = 37, 53
    f, planes = xc.simple(W, H, MIXED, seed=6, **kw)
    info, channels, chunks = exr_file_info(f)
    m_info, m_channels, m_out, m_chunks = xc.read(f)
    # the model reads back what the builder was given
    assert np.array_equal(m_out, xc.pack_planes(planes, W, H, MIXED)) and m_channels == MIXED
    assert (info["width"], info["height"], info["n_channels"], info["compression"], info["line_order"]) == (W, H, 6, kw.get("compression", 3), kw.get("line_order", 0))
    assert info["data_window"] == m_info["data_window"] == (kw.get("x_min", 0), kw.get("y_min", 0), kw.get("x_min", 0) + W - 1, kw.get("y_min", 0) + H - 1)
    assert info["display_window"] == (None if kw.get("display") is False else (0, 0, W - 1, H - 1))
    assert info["long_names"] == int(bool(kw.get("long_names"))) and info["tiled"] == int("tile" in kw)
    tile = kw.get("tile")
    lines = tile[1] if tile else {0: 1, 2: 1, 3: 16}[info["compression"]]
    assert (info["tile_w"], info["tile_h"]) == (tile or (0, 0)) and info["lines_per_chunk"] == lines
    offs, out_len = xc.plane_layout(W, H, MIXED)
    assert info["out_len"] == out_len and out_len > W * H * 16 and [c["plane_off"] for c in channels] == offs and all(o % 16 == 0 for o in offs)
    assert [(c["name"], c["type"], c["sample_bytes"]) for c in channels] == [(n, t, xc.SIZE[t]) for n, t in MIXED]
    assert info["n_chunks"] == len(chunks) == len(m_chunks)
    for c, m in zip(chunks, m_chunks):
        assert (c["off"], c["data_len"], c["raw_len"], c["x"], c["y"], c["w"], c["h"], c["status"]) == (m["off"], m["size"], m["raw_len"], m["x"], m["y"], m["w"], m["h"], 0)
    if kw.get("raw_chunks"):
        assert chunks[1]["data_len"] == chunks[1]["raw_len"] and chunks[0]["data_len"] < chunks[0]["raw_len"]
    if kw.get("line_order") == 1 and not tile:
        assert chunks[0]["off"] > chunks[-1]["off"]  # the table is in the order of the lines, the bodies are not
    if tile == (16, 16):
        assert (chunks[-1]["x"], chunks[-1]["y"], chunks[-1]["w"], chunks[-1]["h"]) == (32, 48, 5, 5)
    # counts only; lists that are too short
    L = _native.lib()
    i2 = _native.ExrInfo()
    assert L.zs_exr_file_info(f, len(f), i2, (_native.ExrChannel * 2)(), 2, None, 0) == ZS_BUF_ERROR and i2.n_channels == 6
    assert L.zs_exr_file_info(f, len(f), i2, None, 0, (_native.ExrChunk * 1)(), 1) == ZS_BUF_ERROR and i2.n_chunks == len(chunks)
    assert L.zs_exr_file_info(f, len(f), None, None, 0, None, 0) == ZS_STREAM_ERROR and L.zs_exr_file_info(f, -1, i2, None, 0, None, 0) == ZS_STREAM_ERROR


def test_edges_of_the_shapes():
    for W, H, comp in ((1, 1, 3), (1, 40, 3), (40, 1, 2), (5, 15, 3), (5, 16, 3), (5, 17, 3), (5, 33, 3)):
        f, planes = xc.simple(W, H, xc.RG, seed=7, compression=comp)
        info, _, chunks = exr_file_info(f)
        lines = 16 if comp == 3 else 1
        assert info["n_chunks"] == -(-H // lines) and [c["h"] for c in chunks] == [min(lines, H - y) for y in range(0, H, lines)]
        assert [c["raw_len"] for c in chunks] == [c["h"] * W * 4 for c in chunks] and np.array_equal(xc.read(f)[2], xc.pack_planes(planes, W, H, xc.RG))


@pytest.mark.parametrize("claim", xc.CLAIMS, ids=[c[0] for c in xc.CLAIMS])
def test_every_error_class_beside_its_nearest_legal_file(claim):
    what, legal, bad, code, message = claim
    assert code_of(legal)[0] == 0, what
    assert code_of(bad)[0] == code, what
    with pytest.raises(ZlibStreamException):
        exr_file_info(bad)


def test_every_prefix_shorter_than_eight_bytes():
    f = xc.CLAIMS[0][1]
    for n in range(8):
        assert code_of(f[:n])[0] == ZS_BUF_ERROR, n


def test_chunk_errors_leave_the_walk_going():
    W, H = 6, 40
    planes = xc.pixels(W, H, xc.RG, seed=8)
    for what, edit, code, _ in xc.CHUNK_CLAIMS:
        f = xc.build(planes, W, H, xc.RG, edit=edit)
        info, _, chunks = exr_file_info(f)
        assert [c["status"] for c in chunks] == [0, code, 0], what
        assert chunks[1]["off"] == 0 and chunks[1]["data_len"] == 0
    # a size of exactly U is the raw form, one more is not
    f = xc.build(planes, W, H, xc.RG, raw_chunks=(1,))
    assert exr_file_info(f)[2][1]["data_len"] == 16 * W * 4
    # a body, a chunk header and an offset that the file ends in
    f = xc.build(planes, W, H, xc.RG)
    _, _, chunks = exr_file_info(f)
    for cut, want in ((len(f) - 1, [0, 0, ZS_BUF_ERROR]), (chunks[2]["off"] - 1, [0, 0, ZS_BUF_ERROR]), (chunks[1]["off"] + chunks[1]["data_len"], [0, 0, ZS_BUF_ERROR]),
                      (chunks[1]["off"] + chunks[1]["data_len"] - 1, [0, ZS_BUF_ERROR, ZS_BUF_ERROR])):
        assert [c["status"] for c in exr_file_info(f[:cut])[2]] == want, cut
    g = bytearray(f)
    table = chunks[0]["off"] - 8 - 24
    g[table + 8:table + 16] = struct.pack("<Q", len(f) + 1)
    assert [c["status"] for c in exr_file_info(g)[2]] == [0, ZS_BUF_ERROR, 0]
    # tiles: the coordinates of the slot
    f = xc.build(xc.pixels(20, 20, xc.RG, seed=9), 20, 20, xc.RG, tile=(16, 16), edit=lambda k, c, n, d: ((c[1], c[0], 0, 0), n, d))
    assert [c["status"] for c in exr_file_info(f)[2]] == [0, ZS_DATA_ERROR, ZS_DATA_ERROR, 0]
    f = xc.build(xc.pixels(20, 20, xc.RG, seed=9), 20, 20, xc.RG, tile=(16, 16), edit=lambda k, c, n, d: ((c[0], c[1], int(k == 3), 0), n, d))
    assert [c["status"] for c in exr_file_info(f)[2]] == [0, 0, 0, ZS_DATA_ERROR]


def image(width=100, height=70, channels=RGBA, **kw):
    return {**dict(planes=0x1000, width=width, height=height, channels=channels), **kw}


def head_bytes(channels, extra=0):
    chl = sum(len(n) + 1 + 16 for n, _ in channels) + 1
    attrs = {"channels": ("chlist", chl), "compression": ("compression", 1), "dataWindow": ("box2i", 16), "displayWindow": ("box2i", 16), "lineOrder": ("lineOrder", 1),
             "pixelAspectRatio": ("float", 4), "screenWindowCenter": ("v2f", 8), "screenWindowWidth": ("float", 4)}
    return 8 + sum(len(n) + 1 + len(t) + 1 + 4 + size for n, (t, size) in attrs.items()) + extra + 1


def test_exr_bound():
    # the head, the table, and per chunk eight bytes and its raw bytes
    assert exr_bound(image(10, 10)) == head_bytes(RGBA) + 8 + 8 + 10 * 10 * 8
    assert exr_bound(image(100, 70)) == head_bytes(RGBA) + 5 * 16 + 100 * 70 * 8
    assert exr_bound(image(100, 70, compression=2)) == exr_bound(image(100, 70, compression=0)) == head_bytes(RGBA) + 70 * 16 + 100 * 70 * 8
    assert exr_bound(image(9, 9, MIXED, extra=xc.attr("owner", "string", b"me"))) == head_bytes(MIXED, 19) + 16 + 81 * 16
    assert exr_bound(image(channels=[("n" * 31, xc.HALF)])) > 0 and exr_bound(image(x_min=-(1 << 31), y_min=-5)) > 0
    for bad in (dict(channels=[("R", 1), ("G", 1)]), dict(channels=[("G", 1), ("G", 1)]), dict(channels=[("n" * 32, 1)]), dict(channels=[("", 1)]), dict(channels=[]),
                dict(channels=[("c%02d" % k, 1) for k in range(65)]), dict(channels=[("G", 3)]), dict(channels=[("G", -1)]), dict(compression=1), dict(compression=4),
                dict(width=0), dict(height=0), dict(width=1 << 16, height=1 << 13), dict(x_min=(1 << 31) - 50), dict(planes=0)):
        with pytest.raises(ValueError):
            exr_bound(image(**bad))
    assert exr_bound(image(channels=[("c%02d" % k, 1) for k in range(64)])) > 0


def test_argument_checks_before_device_work():
    """Without an engine every call ends in ZS_STREAM_ERROR at its first check; the bindings refuse what they can see."""
    legal = xc.CLAIMS[0][1]
    with pytest.raises(ValueError):
        exr_encode(None, [image()], [0x2000], [1 << 20])
    with pytest.raises(ValueError):
        exr_encode(None, [image()], [0x2000], [])
    with pytest.raises(ValueError):
        exr_decode_files(None, [legal], [0x2000], [1 << 20])
    with pytest.raises(ValueError):
        exr_decode_files(None, [legal], [0], [1 << 20])
    with pytest.raises(ValueError):
        exr_decode_files(None, [legal], [0x2000], [-1])
    with pytest.raises(ValueError):
        exr_unpredict(None, [0x1000], [0x2000], [4])
    with pytest.raises(ValueError):
        exr_predict(None, [0x1000], [0x2000], [4, 4])
    assert exr_encode(None, [], [], []) == (0, [], []) and exr_decode_files(None, [], [], []) == (0, [], [], [])
    # (a null context is the first check: the lengths' own are seen on the device, tests/test_gpu_exr.py)
    VP = ctypes.c_void_p * 1
    assert _native.lib().zs_exr_unpredict_batch_device(None, 1, VP(0x1000), VP(0x2000), (ctypes.c_int64 * 1)(4), None) == ZS_STREAM_ERROR


def test_builder_streams_are_zlib_streams():
    """The yardstick itself: a compressed chunk of a built file is zlib's stream of the predicted raw bytes."""
    f, planes = xc.simple(37, 20, RGBA, seed=10)
    _, _, _, chunks = xc.read(f)
    for c in chunks:
        raw = xc.chunk_raw(planes, RGBA, c["x"], c["y"], c["w"], c["h"])
        assert c["size"] < c["raw_len"] and zlib.decompress(f[c["off"]:c["off"] + c["size"]]) == xc.predict(raw)
