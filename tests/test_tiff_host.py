"""The host side of the TIFF calls, no GPU: the container rules of zlibstream_amd/csrc/zs_tiff.h and the predictor kernels'
per-lane step run by tests/cpp/test_tiff_walk.cpp under the address and undefined-behaviour sanitizers, tiff_file_info against
Pillow's tag_v2 on the golden files libtiff wrote and against tests/tiff_cases.py on built ones, every error class beside its
nearest legal file, tiff_bound, and the argument checks of the device calls that are decided before any device work."""
import io
import os
import subprocess

import numpy as np
import pytest

import tiff_cases as tc
from zlibstream_amd import ZlibStreamException, _native, deflate_bound, tiff_bound, tiff_decode_files, tiff_encode, tiff_file_info, tiff_predict, tiff_unpredict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff")
ZS_STREAM_ERROR, ZS_DATA_ERROR, ZS_BUF_ERROR = -2, -3, -5


def golden(name):
    return open(os.path.join(GOLDEN, name + ".tif"), "rb").read()


def code_of(data, page=0):
    """zs_tiff_file_info's return code and the info as far as it got."""
    data = bytes(data)
    info = _native.TiffInfo()
    return _native.lib().zs_tiff_file_info(data, len(data), page, info, None, 0), info


def small_files():
    rgb, gray16 = tc.pixels(37, 53, 3, 8, seed=3), tc.pixels(21, 40, 1, 16, seed=4)
    two = tc.build([tc.page(rgb, 37, 3, 8, predictor=2, tile=(16, 16)), tc.page(gray16, 21, 1, 16, predictor=2, rows_per_strip=7)])
    return [tc.simple(rgb, 37, 3, 8, predictor=2, rows_per_strip=10), tc.simple(gray16, 21, 1, 16, order=">", big=True, tile=(16, 32), odd_offsets=True), two]


def test_shared_tiff_rules_on_the_host_under_sanitizers():
    """tests/cpp/test_tiff_walk.cpp, a stand-alone program built with -fsanitize=address,undefined: the walk on every prefix of
    three built files and two that libtiff wrote, each in a heap block of exactly its length, on every page and one behind the
    last; the writer's head read back; the kernels' per-lane step over a model of the wave against a scalar loop."""
    build = os.path.join(ROOT, "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_tiff_walk")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_tiff_walk.cpp")], check=True)
    paths = [os.path.join(GOLDEN, "rgb_p2.tif"), os.path.join(GOLDEN, "bilevel.tif")]
    for k, data in enumerate(small_files()):
        paths.append(os.path.join(build, "test_tiff_walk_%d.tif" % k))
        with open(paths[-1], "wb") as f:
            f.write(data)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("name", [g[0] for g in tc.GOLDEN])
def test_file_info_on_the_golden_files(name):
    """What libtiff wrote, against the pixels' own dimensions (always) and against Pillow's reading of the tags (where Pillow is
    installed)."""
    data = golden(name)
    w, h, spp, bits, fmt, predictor = tc.golden_dims(name)
    info, chunks = tiff_file_info(data)
    assert (info["width"], info["height"], info["spp"], info["bits"], info["predictor"]) == (w, h, spp, bits, predictor)
    assert info["compression"] == 8 and info["n_pages"] == 1 and info["big_endian"] == 0 and info["bigtiff"] == 0 and info["tiled"] == 0
    assert info["row_bytes"] == tc.row_bytes(w, spp, bits) and info["out_len"] == h * info["row_bytes"] and info["chunk_w"] == w
    assert info["n_chunks"] == len(chunks) == -(-h // info["chunk_h"]) and info["sample_format"] == fmt
    assert info["extra_samples"] == (1 if name.startswith(("la", "rgba")) else 0)
    y = 0
    for c in chunks:
        assert (c["x"], c["y"], c["w"], c["status"]) == (0, y, w, 0) and c["off"] + c["comp_len"] <= len(data)
        y += c["h"]
    assert y == h
    Image = pytest.importorskip("PIL.Image")
    t = Image.open(io.BytesIO(data)).tag_v2
    assert (t[256], t[257], t[259], t[262], t.get(277, 1)) == (info["width"], info["height"], info["compression"], info["photometric"], info["spp"])
    assert t[258] == (info["bits"],) * info["spp"] and t.get(317, 1) == info["predictor"] and t[278] == info["chunk_h"]
    assert list(t[273]) == [c["off"] for c in chunks] and list(t[279]) == [c["comp_len"] for c in chunks]
    assert t.get(339, (1,))[0] == info["sample_format"] and t.get(274, 1) == info["orientation"]
    if info["extra_samples"]:
        assert len(t[338]) == info["extra_samples"] and t[338][0] == info["extra_kind"]


@pytest.mark.parametrize("order", ["<", ">"])
@pytest.mark.parametrize("big", [False, True])
def test_file_info_on_built_files(order, big):
    rows = tc.pixels(37, 53, 4, 16, seed=5)
    # strips: the default RowsPerStrip is one strip; a short last strip; SHORT and LONG dimensions
    f = tc.simple(rows, 37, 4, 16, order=order, big=big, predictor=2, extra=[2])
    info, chunks = tiff_file_info(f)
    assert (info["n_chunks"], info["chunk_h"], info["big_endian"], info["bigtiff"]) == (1, 53, int(order == ">"), int(big))
    assert (info["extra_samples"], info["extra_kind"], info["photometric"], info["planar"], info["orientation"]) == (1, 2, 2, 1, 1)
    f = tc.simple(rows, 37, 4, 16, order=order, big=big, rows_per_strip=10, tags={256: (3, [37]), 257: (3, [53])})
    info, chunks = tiff_file_info(f)
    assert info["n_chunks"] == 6 and [c["h"] for c in chunks] == [10] * 5 + [3] and [c["y"] for c in chunks] == list(range(0, 60, 10))
    ifds, _ = tc.read_ifds(f)
    assert [c["off"] for c in chunks] == ifds[0][273] and [c["comp_len"] for c in chunks] == ifds[0][279]
    # tiles: 16 x 32 on 37 x 53 is 3 x 2, the right column 5 wide and the bottom row 21 high
    f = tc.simple(rows, 37, 4, 16, order=order, big=big, tile=(16, 32), odd_offsets=True)
    info, chunks = tiff_file_info(f)
    assert (info["tiled"], info["chunk_w"], info["chunk_h"], info["n_chunks"]) == (1, 16, 32, 6)
    assert [(c["x"], c["y"], c["w"], c["h"]) for c in chunks] == [(0, 0, 16, 32), (16, 0, 16, 32), (32, 0, 5, 32), (0, 32, 16, 21), (16, 32, 16, 21), (32, 32, 5, 21)]
    assert all(c["off"] % 2 == 1 and c["status"] == 0 for c in chunks)
    # the second page of two, and the page behind the last
    gray = tc.pixels(20, 9, 1, 8, seed=6)
    two = tc.build([tc.page(rows, 37, 4, 16, order=order), tc.page(gray, 20, 1, 8, order=order, compression=1)], order=order, big=big)
    info, chunks = tiff_file_info(two, page=1)
    assert (info["n_pages"], info["width"], info["height"], info["bits"], info["compression"], chunks[0]["comp_len"]) == (2, 20, 9, 8, 1, 180)
    rc, info = code_of(two, page=2)
    assert rc == ZS_DATA_ERROR and info.n_pages == 2
    # the chunks' cap: the counts alone, and a list that is too short
    n = _native.lib().zs_tiff_file_info(f, len(f), 0, info, (_native.TiffChunk * 2)(), 2)
    assert n == ZS_BUF_ERROR and info.n_chunks == 6


def legal(**kw):
    return tc.simple(tc.pixels(40, 20, 1, 8, seed=7), 40, 1, 8, rows_per_strip=8, **kw)


def test_every_error_class_beside_its_nearest_legal_file():
    assert code_of(legal())[0] == 0 and code_of(legal(tile=(16, 16)))[0] == 0
    data = lambda tags: legal(tags=tags)  # noqa: E731
    # ZS_BUF_ERROR: shorter than the header
    for n in range(8):
        assert code_of(legal()[:n])[0] == ZS_BUF_ERROR, n
    assert code_of(legal(big=True)[:15])[0] == ZS_BUF_ERROR
    # magic and version
    f = bytearray(legal())
    for at, v in ((0, b"JJ"), (0, b"IM"), (2, b"\x29\0"), (2, b"\x2c\0")):
        g = bytearray(f)
        g[at:at + 2] = v
        assert code_of(g)[0] == ZS_DATA_ERROR, (at, v)
    # the IFD, or a value, out of the file; a chain that loops
    g = bytearray(f)
    g[4:8] = (len(f) - 5).to_bytes(4, "little")
    assert code_of(g)[0] == ZS_DATA_ERROR
    assert code_of(f[:8 + 2 + 12 * 3])[0] == ZS_DATA_ERROR  # the file ends inside the IFD
    info, _ = tiff_file_info(bytes(f))
    assert info["n_chunks"] == 3
    ifds, _ = tc.read_ifds(bytes(f))
    values_at = 8 + 2 + 12 * len(ifds[0]) + 4  # the three offsets, then the three byte counts
    assert code_of(f[:values_at + 12 + 11])[0] == ZS_DATA_ERROR and code_of(f[:values_at + 24])[0] == 0
    assert code_of(tc.build([tc.page(tc.pixels(8, 8), 8)], loop=True))[0] == ZS_DATA_ERROR
    # required tags, array lengths
    for tag in (256, 257, 273, 279):
        assert code_of(legal(tags={tag: None}))[0] == ZS_DATA_ERROR, tag
    assert code_of(legal(tile=(16, 16), tags={322: None}))[0] == ZS_DATA_ERROR and code_of(legal(tile=(16, 16), tags={325: None}))[0] == ZS_DATA_ERROR
    assert code_of(data({279: (4, [1, 2])}))[0] == ZS_DATA_ERROR and code_of(data({278: (3, [4])}))[0] == ZS_DATA_ERROR
    # what is not supported, each beside the nearest value that is
    for tags, ok in (({259: (3, [5])}, {259: (3, [32946])}), ({317: (3, [4])}, {317: (3, [2])}), ({284: (3, [2]), 277: (3, [2]), 258: (3, [8, 8])}, {284: (3, [2])}),
                     ({258: (3, [12])}, {258: (3, [8])}), ({258: (3, [8, 16]), 277: (3, [2])}, {258: (3, [8, 8]), 277: (3, [2])}), ({266: (3, [2])}, {266: (3, [1])}),
                     ({262: (3, [6])}, {262: (3, [5])}), ({277: (3, [9]), 258: (3, [8] * 9)}, {277: (3, [8]), 258: (3, [8] * 8)}),
                     ({256: (4, [0])}, {256: (4, [41])}), ({278: (3, [0])}, {278: (3, [8])})):
        assert code_of(data(tags))[0] == ZS_DATA_ERROR, tags
        assert code_of(data(ok))[0] == 0, ok
    assert code_of(legal(tile=(16, 16), tags={322: (3, [24])}))[0] == ZS_DATA_ERROR  # a tile width that is no multiple of 16
    # predictor 2 below 8 bits (libtiff refuses it too), predictor 3 on integers
    bi = tc.pixels(40, 20, 1, 1, seed=8)
    assert code_of(tc.simple(bi, 40, 1, 1))[0] == 0 and code_of(tc.simple(bi, 40, 1, 1, tags={317: (3, [2])}))[0] == ZS_DATA_ERROR
    fl = tc.pixels(10, 5, 1, 32, seed=9, fmt=3)
    assert code_of(tc.simple(fl, 10, 1, 32, fmt=3, predictor=3))[0] == 0
    assert code_of(tc.simple(fl, 10, 1, 32, fmt=1, predictor=3))[0] == ZS_DATA_ERROR
    assert code_of(tc.simple(tc.pixels(10, 5, 1, 16), 10, 1, 16, tags={317: (3, [3])}))[0] == ZS_DATA_ERROR
    # pixels above 2 GiB - 1 KiB
    assert code_of(data({256: (4, [1 << 20]), 257: (4, [1 << 12]), 278: (4, [1 << 12]), 279: (4, [3]), 273: (4, [8])}))[0] == ZS_DATA_ERROR
    # per chunk: a body that the file ends in, the walk going on
    f = legal()
    info, chunks = tiff_file_info(f[:chunks_end(f, 1) + 1])
    assert [c["status"] for c in chunks] == [0, 0, ZS_BUF_ERROR]
    with pytest.raises(ZlibStreamException):
        tiff_file_info(b"II*\0")


def chunks_end(f, k):
    _, chunks = tiff_file_info(f)
    return chunks[k]["off"] + chunks[k]["comp_len"]


def image(width=100, height=70, **kw):
    return dict(pixels=0x1000, width=width, height=height, **kw)


def test_tiff_bound():
    # one strip: head = 8 + 2 + 12 tags x 12 + 4, no longer values
    assert tiff_bound(image(10, 10)) == 158 + 2 + deflate_bound(100) + 1
    # rows_per_strip 0: strips of about 256 KiB
    b = tiff_bound(image(1024, 1000, bits=8, spp=1))
    head = 160 + 2 * 4 * 4
    assert b == head + 3 * (deflate_bound(256 << 10) + 1) + deflate_bound(232 * 1024) + 1
    # tiles: whole tiles, also at the edges; spp 3: BitsPerSample and SampleFormat lie behind the IFD
    b = tiff_bound(image(100, 70, spp=3, bits=16, predictor=2, tile_width=32, tile_height=16))
    assert b == (8 + 2 + 13 * 12 + 4 + 12 + 2) // 4 * 4 + 2 * 4 * 20 + 20 * (deflate_bound(32 * 16 * 6) + 1)
    for bad in (dict(bits=12), dict(spp=9), dict(spp=0), dict(predictor=2, bits=4), dict(predictor=3, bits=32), dict(predictor=3, bits=16, sample_format=3),
                dict(tile_width=16), dict(tile_width=24, tile_height=16), dict(photometric=6), dict(extra_samples=1), dict(rows_per_strip=-1), dict(width=0),
                dict(width=1 << 20, height=1 << 12), dict(sample_format=0)):
        with pytest.raises(ValueError):
            tiff_bound(image(**bad))
    with pytest.raises(ValueError):
        tiff_bound(dict(pixels=0, width=4, height=4))
    assert tiff_bound(image(predictor=3, bits=32, sample_format=3)) > 0 and tiff_bound(image(spp=2, extra_samples=1, extra_kind=2)) > 0


def test_argument_checks_before_device_work():
    """Without an engine every call ends in ZS_STREAM_ERROR at its first check; the bindings refuse what they can see."""
    with pytest.raises(ValueError):
        tiff_encode(None, [image()], [0x2000], [1 << 20])
    with pytest.raises(ValueError):
        tiff_encode(None, [image()], [0x2000], [])
    with pytest.raises(ValueError):
        tiff_decode_files(None, [legal()], [0x2000], [1 << 20])
    with pytest.raises(ValueError):
        tiff_decode_files(None, [legal()], [0], [1 << 20])
    with pytest.raises(ValueError):
        tiff_decode_files(None, [legal()], [0x2000], [1 << 20], pages=[-1])
    with pytest.raises(ValueError):
        tiff_unpredict(None, [0x1000], [0x2000], [4], [4], [8], [1], [2])
    with pytest.raises(ValueError):
        tiff_predict(None, [0x1000], [0x2000], [4], [4], [8], [1], [2, 2])
    assert tiff_encode(None, [], [], []) == (0, [], []) and tiff_decode_files(None, [], [], []) == (0, [], [], [])


def test_builder_and_reader_agree_with_pillow():
    """The yardsticks themselves: Pillow reads what the builder writes, for the shapes Pillow handles."""
    Image = pytest.importorskip("PIL.Image")
    for spp, mode in ((1, "L"), (3, "RGB"), (4, "RGBA")):
        rows = tc.pixels(37, 53, spp, 8, seed=10)
        for order in "<>":
            for kw in (dict(predictor=2, tile=(16, 16)), dict(predictor=1, rows_per_strip=10), dict(predictor=2, rows_per_strip=10, pad_last_strip=True)):
                f = tc.simple(rows, 37, spp, 8, order=order, extra=[2] if spp == 4 else None, **kw)
                im = Image.open(io.BytesIO(f))
                assert im.mode == mode and np.array_equal(np.asarray(im).reshape(53, -1), rows)
                assert np.array_equal(tc.read(f)[1], rows)
    rows = tc.pixels(37, 53, 1, 16, seed=11)
    for order in "<>":
        f = tc.simple(rows, 37, 1, 16, order=order, predictor=2, rows_per_strip=10)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))).astype("<u2").view(np.uint8).reshape(53, -1), rows)
