"""The host side of the chunked-array calls, no GPU: the geometry, item decomposition and per-lane steps of
zlibstream_amd/csrc/zs_chunk.h run by tests/cpp/test_chunk_rows.cpp under the address and undefined-behaviour sanitizers,
chunk_grid_info against tests/chunk_cases.py with every grid rule from both sides, chunks_bound, the argument checks that are
decided before any device work, zarr_v2_grid on hand-written .zarray documents, and the model against itself."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import chunk_cases as cc
from zlibstream_amd import (_native, chunk_grid_info, chunks_bound, chunks_decode, chunks_encode, shuffle, unshuffle, wrap_bound, zarr_v2_grid, WRAP_GZIP, WRAP_RAW,
                            WRAP_ZLIB)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS_STREAM_ERROR = -2


def test_shared_chunk_rules_on_the_host_under_sanitizers():
    """tests/cpp/test_chunk_rows.cpp, a stand-alone program built with -fsanitize=address,undefined: every item and lane of the
    place, gather and survey steps against a scalar loop, ranks 1..4, elem_size 1..16, each byte written exactly once, every
    buffer a heap block of exactly its length."""
    build = os.path.join(ROOT, "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_chunk_rows")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_chunk_rows.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), (r.stdout[-2000:], r.stderr[-3000:])


def test_the_model_against_itself():
    """The yardstick: shuffle is a transpose with HDF5's leftover rule, chunk_of pads with fill, place undoes chunk_of."""
    assert cc.shuffle(bytes([1, 2, 3, 4, 5, 6, 7]), 2) == bytes([1, 3, 5, 2, 4, 6, 7])
    assert cc.unshuffle(bytes([1, 3, 5, 2, 4, 6, 7]), 2) == bytes([1, 2, 3, 4, 5, 6, 7])
    assert cc.shuffle(b"abc", 4) == b"abc" and cc.shuffle(b"", 3) == b""
    g = cc.grid((3, 5), (2, 4), 2, fill=b"\xAA\xBB")
    data = bytes(range(30))
    assert cc.cells(g) == (2, 2) and cc.n_chunks(g) == 4 and cc.chunk_bytes(g) == 16 and cc.array_bytes(g) == 30
    # chunk 1: rows 0..1, column 4 and three columns of padding
    assert cc.chunk_of(data, g, 1, shuffled=False) == bytes([8, 9]) + b"\xAA\xBB" * 3 + bytes([18, 19]) + b"\xAA\xBB" * 3
    assert cc.chunk_of(data, g, 1) == cc.shuffle(cc.chunk_of(data, g, 1, shuffled=False), 2)
    chunks = [cc.chunk_of(data, g, c, shuffled=False) for c in range(4)]
    assert cc.place(chunks, g) == data
    sent = b"\xEE" * 30
    want = bytearray(data)
    want[8:10] = want[18:20] = b"\xAA\xBB"
    assert cc.place([chunks[0], None, chunks[2], chunks[3]], g, into=sent) == bytes(want)
    want[8:10] = want[18:20] = b"\xEE\xEE"
    assert cc.place([chunks[0], "skip", chunks[2], chunks[3]], g, into=sent) == bytes(want)
    for wrap in (WRAP_ZLIB, WRAP_RAW, WRAP_GZIP):
        assert cc.decompress(cc.compress(data, wrap), wrap) == (data, 0)


def grids_for_info():
    out = []
    for es in (1, 2, 3, 4, 8, 16):
        out += cc.edge_grids(es)
    out += [cc.grid((1,), (1,), 1), cc.grid((3, 50), (8, 600), 4), cc.grid((70001,), (70001,), 4), cc.grid((2,) * 8, (1,) * 8, 16),
            cc.grid((1 << 40, 1 << 20), (1 << 20, 1 << 10), 4)]
    return out


def test_chunk_grid_info_against_the_model():
    for g in grids_for_info():
        assert chunk_grid_info(g) == (cc.n_chunks(g), cc.chunk_bytes(g), cc.array_bytes(g)), g
    # the largest products that stay inside int64, and the first that leave it
    assert chunk_grid_info(cc.grid(((1 << 62) - 1,), (1,), 2)) == ((1 << 62) - 1, 2, (1 << 63) - 2)
    with pytest.raises(ValueError):
        chunk_grid_info(cc.grid((1 << 62,), (1,), 2))
    assert chunk_grid_info(cc.grid((1,), ((1 << 59) - 1,), 16))[1] == (1 << 63) - 16
    with pytest.raises(ValueError):
        chunk_grid_info(cc.grid((1,), (1 << 59,), 16))
    assert chunk_grid_info(cc.grid((1 << 31, 1 << 31), (1, 1), 1))[0] == 1 << 62
    with pytest.raises(ValueError):
        chunk_grid_info(cc.grid((1 << 32, 1 << 31), (1, 1), 1))


@pytest.mark.parametrize("good,bad", [
    (dict(shape=(5,), chunks=(2,)), dict(shape=(), chunks=())),                         # rank 1 / rank 0
    (dict(shape=(2,) * 8, chunks=(1,) * 8), dict(shape=(2,) * 9, chunks=(1,) * 9)),   # rank 8 / rank 9
    (dict(elem_size=1), dict(elem_size=0)), (dict(elem_size=16), dict(elem_size=17)),
    (dict(shape=(1, 1)), dict(shape=(1, 0))), (dict(chunks=(1, 1)), dict(chunks=(0, 1))), (dict(shape=(1, 1)), dict(shape=(-1, 1))),
    (dict(wrap=WRAP_GZIP), dict(wrap=3)), (dict(wrap=WRAP_ZLIB), dict(wrap=-1)),
])
def test_each_grid_rule_from_both_sides(good, bad):
    base = dict(shape=(5, 7), chunks=(2, 3), elem_size=4, fill=None)
    for change, legal in ((good, True), (bad, False)):
        d = {**base, **change}
        g = {"shape": d["shape"], "chunks": d["chunks"], "elem_size": d["elem_size"], "wrap": d.get("wrap", 0)}
        if legal:
            assert chunk_grid_info(g)[0] >= 1 and chunks_bound(g) > 0
        else:
            with pytest.raises(ValueError):
                chunk_grid_info(g)
            with pytest.raises(ValueError):
                chunks_bound(g)
    # (the raw call answers ZS_STREAM_ERROR, and for a null grid too)
    assert _native.lib().zs_chunk_grid_info(None, None, None, None) == ZS_STREAM_ERROR and _native.lib().zs_chunks_bound(None) == -1


def test_chunks_bound():
    for g in grids_for_info():
        for wrap in (WRAP_ZLIB, WRAP_RAW, WRAP_GZIP):
            g = {**g, "wrap": wrap}
            assert chunks_bound(g) == cc.n_chunks(g) * wrap_bound(cc.chunk_bytes(g), wrap)
    assert chunk_grid_info(cc.grid((1 << 62,), (1,), 1))[0] == 1 << 62
    with pytest.raises(ValueError):  # (2^62 chunks of a byte: the grid is legal, the bound leaves int64)
        chunks_bound(cc.grid((1 << 62,), (1,), 1))


def test_argument_checks_before_device_work():
    """Without an engine every call ends in ZS_STREAM_ERROR at its first check; the bindings refuse what they can see."""
    g = cc.grid((5, 7), (2, 3), 4)
    data = cc.random_array(g, 1)
    enc = cc.encoded_chunks(data, g)
    with pytest.raises(ValueError):
        chunks_decode(None, [g], [enc], [0x2000], [1 << 20])
    with pytest.raises(ValueError):
        chunks_decode(None, [g], [enc[:-1]], [0x2000], [1 << 20])  # a chunk too few
    with pytest.raises(ValueError):
        chunks_decode(None, [g], [enc], [0x2000], [])
    with pytest.raises(ValueError):
        chunks_decode(None, [{**g, "elem_size": 17}], [enc], [0x2000], [1 << 20])
    with pytest.raises(ValueError):
        chunks_decode(None, [{**g, "order": "F"}], [enc], [0x2000], [1 << 20])
    with pytest.raises(ValueError):
        chunks_decode(None, [{**g, "fill": b"\0"}], [enc], [0x2000], [1 << 20])
    with pytest.raises(ValueError):
        chunks_encode(None, [g], [0x1000], [0x2000], [1 << 20])
    with pytest.raises(ValueError):
        chunks_encode(None, [g], [0x1000], [0x2000], [])
    with pytest.raises(ValueError):
        chunks_encode(None, [{**g, "shape": (5, 0)}], [0x1000], [0x2000], [1 << 20])
    with pytest.raises(ValueError):
        shuffle(None, [0x1000], [0x2000], [8], [4])
    with pytest.raises(ValueError):
        unshuffle(None, [0x1000], [0x2000], [8, 8], [4])
    assert chunks_decode(None, [], [], [], []) == (0, [], []) and chunks_encode(None, [], [], [], []) == (0, [], [], [])
    assert shuffle(None, [], [], [], []) is None
    L = _native.lib()
    VP = ctypes.c_void_p * 1
    assert L.zs_shuffle_batch_device(None, 1, VP(0x1000), VP(0x2000), (ctypes.c_int64 * 1)(4), (ctypes.c_int * 1)(2), None) == ZS_STREAM_ERROR
    assert L.zs_chunks_decode_batch(None, 0, None, None, None, None, None, None, None) == ZS_STREAM_ERROR
    assert ctypes.sizeof(_native.ChunkGrid) == 160 and ctypes.sizeof(_native.ChunkRef) == 24


# ------------------------------------------------------------------ zarr_v2_grid
ACCEPTED = [
    (cc.zarray((10, 20), (4, 5)), dict(shape=(10, 20), chunks=(4, 5), elem_size=4, shuffle=False, wrap=WRAP_ZLIB, fill=bytes(4), stored=False, level=6)),
    (cc.zarray((7,), (3,), dtype="<f8", compressor={"id": "gzip", "level": 1}), dict(elem_size=8, wrap=WRAP_GZIP, level=1)),
    (cc.zarray((7,), (3,), dtype="|u1", compressor=None), dict(elem_size=1, stored=True, level=None)),
    (cc.zarray((7,), (3,), dtype="|b1"), dict(elem_size=1)),
    (cc.zarray((7,), (3,), dtype=">i1"), dict(elem_size=1)),  # (a single byte has no order)
    (cc.zarray((7,), (3,), dtype="<c16"), dict(elem_size=16)),
    (cc.zarray((7,), (3,), dtype="<M8[ns]"), dict(elem_size=8)),
    (cc.zarray((7,), (3,), dtype="|S5", fill_value=None), dict(elem_size=5, fill=bytes(5))),
    (cc.zarray((7,), (3,), dtype="<i2", filters=[{"id": "shuffle", "elementsize": 2}]), dict(elem_size=2, shuffle=True)),
    (cc.zarray((7,), (3,), filters=[]), dict(shuffle=False)),
    (cc.zarray((7,), (3,), fill_value=1.5), dict(fill=np.float32(1.5).tobytes())),
    (cc.zarray((7,), (3,), fill_value="NaN"), dict(fill=np.float32("nan").tobytes())),
    (cc.zarray((7,), (3,), fill_value="-Infinity"), dict(fill=np.float32("-inf").tobytes())),
    (cc.zarray((7,), (3,), dtype="<i8", fill_value=-2), dict(fill=np.int64(-2).tobytes())),
    (cc.zarray((7,), (3,), fill_value=None), dict(fill=bytes(4))),
    (cc.zarray((7,), (3,), dimension_separator="/"), dict(shape=(7,))),
    (cc.zarray((2,) * 8, (1,) * 8), dict(shape=(2,) * 8)),
]
REJECTED = [
    ("zarr_format", cc.zarray((7,), (3,), zarr_format=3)), ("zarr_format", {k: v for k, v in cc.zarray((7,), (3,)).items() if k != "zarr_format"}),
    ("order", cc.zarray((7,), (3,), order="F")),
    ("dtype", cc.zarray((7,), (3,), dtype=">f4")), ("dtype", cc.zarray((7,), (3,), dtype="|O")), ("dtype", cc.zarray((7,), (3,), dtype=[["a", "<i4"], ["b", "<f4"]])),
    ("dtype", cc.zarray((7,), (3,), dtype="<U4")), ("dtype", cc.zarray((7,), (3,), dtype="|S17")), ("dtype", cc.zarray((7,), (3,), dtype="f4")),
    ("shape", cc.zarray((7, 0), (3, 1))), ("shape", cc.zarray((), ())), ("shape", cc.zarray((2,) * 9, (1,) * 9)),
    ("chunks", cc.zarray((7, 2), (3,))), ("chunks", cc.zarray((7,), (0,))),
    ("compressor", cc.zarray((7,), (3,), compressor={"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1})), ("compressor", cc.zarray((7,), (3,), compressor={"id": "zstd", "level": 1})),
    ("filters", cc.zarray((7,), (3,), filters=[{"id": "delta", "dtype": "<f4"}])), ("filters", cc.zarray((7,), (3,), filters=[{"id": "shuffle", "elementsize": 2}])),
    ("filters", cc.zarray((7,), (3,), filters=[{"id": "shuffle", "elementsize": 4}, {"id": "shuffle", "elementsize": 4}])),
    ("fill_value", cc.zarray((7,), (3,), dtype="<i4", fill_value="abc")), ("fill_value", cc.zarray((7,), (3,), fill_value=[1, 2])),
]


@pytest.mark.parametrize("k", range(len(ACCEPTED)))
def test_zarr_v2_grid_accepts(k):
    doc, want = ACCEPTED[k]
    for form in (doc, json.dumps(doc), json.dumps(doc).encode()):
        g = zarr_v2_grid(form)
        for key, v in want.items():
            assert g[key] == v, (key, g)
    n, cb, ab = chunk_grid_info(g)  # (what it makes is a grid the library takes)
    assert (n, cb, ab) == (cc.n_chunks(g), cc.chunk_bytes(g), cc.array_bytes(g))


@pytest.mark.parametrize("k", range(len(REJECTED)))
def test_zarr_v2_grid_rejects_naming_the_field(k):
    field, doc = REJECTED[k]
    with pytest.raises(ValueError, match="zarr_v2_grid: %s:" % field):
        zarr_v2_grid(json.dumps(doc))
