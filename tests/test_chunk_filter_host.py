"""The host side of the chunk filters (Fletcher-32, delta, big-endian elements), no GPU: the closed form of the checksum against
the literal loop of H5_checksum_fletcher32, tests/cpp/test_chunk_filters.cpp under the address and undefined-behaviour sanitizers,
the model of tests/chunk_filter_cases.py against itself, chunks_filters_bound and every rejected (grid, filters) pair beside its
nearest legal one, the argument checks decided before any device work, and zarr_v2_filters on hand-written .zarray documents."""
import ctypes
import itertools
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import chunk_cases as cc
import chunk_filter_cases as fc
from zlibstream_amd import (_native, chunks_bound, chunks_decode, chunks_encode, chunks_filters_bound, delta_decode, delta_encode, fletcher32, zarr_v2_filters, zarr_v2_grid,
                            DELTA_TILE, FLETCHER32_TILE, WRAP_GZIP, WRAP_ZLIB)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS_STREAM_ERROR = -2


def test_filter_rules_on_the_host_under_sanitizers():
    """tests/cpp/test_chunk_filters.cpp, a stand-alone program built with -fsanitize=address,undefined: the checksum's per-lane
    step and combine rule against the literal loop, the delta steps and the byte reversal of place and gather against scalar
    loops, every buffer a heap block of exactly its length."""
    build = os.path.join(ROOT, "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_chunk_filters")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_chunk_filters.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), (r.stdout[-2000:], r.stderr[-3000:])


# ------------------------------------------------------------------ the closed form against the loop
def closed_form_inputs():
    alphabet = (0x00, 0x01, 0xFE, 0xFF)
    for n in range(6):
        for v in itertools.product(alphabet, repeat=n):
            yield bytes(v)
    for n in (0, 1, 2, 3, 719, 720, 721, 722, 1439, 1440, 1441, 1442, 65534, 65535, 65536, 65537, 65538):
        yield bytes(n)
        yield b"\xff" * n
    rng = np.random.default_rng(77)
    for _ in range(200):
        yield rng.integers(0, 256, int(rng.integers(0, 4097)), dtype=np.uint8).tobytes()


def test_fletcher32_closed_form_against_the_loop():
    """Each sum is its exact value modulo 65535, a residue of 0 reading as 0xffff unless every word was zero."""
    for d in closed_form_inputs():
        want = fc.fletcher32_loop(d)
        assert fc.fletcher32_fast(d) == want, (len(d), d[:8])
        if len(d) <= 4096:
            assert fc.fletcher32_closed(d) == want, (len(d), d[:8])
    assert fc.fletcher32_loop(b"") == 0 and fc.fletcher32_loop(bytes(7)) == 0 and fc.fletcher32_loop(b"\xff\xff") == 0xFFFFFFFF
    assert fc.fletcher32_loop(b"\x00\x01") == 0x00010001 and fc.fletcher32_loop(b"\x01") == 0x01000100


def test_fletcher32_combine_rule_at_every_cut():
    """(a1, a2) over n words then (b1, b2) over m words: (a1 + b1, a2 + m a1 + b2), with the any-non-zero flag."""
    rng = np.random.default_rng(78)
    for d in (rng.integers(0, 256, 1441, dtype=np.uint8).tobytes(), b"\xff" * 722, bytes(300) + rng.integers(0, 256, 301, dtype=np.uint8).tobytes()):
        want = fc.fletcher32_loop(d)
        for cut in range(0, len(d) + 1, 2):
            a, b = fc.fletcher32_sums(d[:cut]), fc.fletcher32_sums(d[cut:])
            assert fc.fletcher32_finish(fc.fletcher32_combine(a, b, (len(d) - cut + 1) // 2)) == want, (len(d), cut)


def test_the_model_against_itself():
    """Delta wraps and undoes itself, the byte order is a reversal, and the chain of a chunk is delta, byte order, shuffle."""
    x = struct.pack("<4H", 0xFFFF, 1, 0, 0x8000)
    assert fc.delta_encode(x, 2) == struct.pack("<4H", 0xFFFF, 2, 0xFFFF, 0x8000) and fc.delta_decode(fc.delta_encode(x, 2), 2) == x
    assert fc.delta_encode(b"\x05\x07\x06\x09", 1) == b"\x05\x02\xff\x03" and fc.delta_encode(b"abcde", 4) == b"abcde" and fc.delta_encode(b"", 8) == b""
    assert fc.delta_encode(x + b"z", 2) == fc.delta_encode(x, 2) + b"z" and fc.delta_decode(fc.delta_encode(x, 2) + b"z", 2) == x + b"z"
    assert fc.byteswap(bytes(range(8)), 4) == bytes([3, 2, 1, 0, 7, 6, 5, 4])
    g = cc.grid((3,), (2,), 2, fill=b"\xAA\xBB")
    data = struct.pack("<3H", 0x0102, 0x0104, 0x0101)
    f = fc.filters(delta=1, byte_order=1)
    # chunk 1: element 0x0101 and one of fill (0xBBAA); differences 0x0101, 0xBAA9; big-endian; planes of the stored bytes
    assert fc.filtered_chunk(data, g, f, 1) == bytes([0x01, 0xBA, 0x01, 0xA9])
    assert fc.filtered_chunk(data, g, f, 1, shuffled=False) == bytes([0x01, 0x01, 0xBA, 0xA9])
    for f in fc.all_filters():
        for shuffle in (True, False):
            g = cc.grid((5, 7), (2, 3), 4, shuffle=shuffle)
            data = cc.random_array(g, 3)
            enc = fc.encoded_chunks(data, g, f)
            assert cc.place([fc.decoded_chunk(e, g, f) for e in enc], g) == data
            assert all((len(e) - len(cc.compress(fc.filtered_chunk(data, g, f, c), 0))) == 4 * f["fletcher32"] for c, e in enumerate(enc))


# ------------------------------------------------------------------ bounds and rules
def test_chunks_filters_bound():
    for g in (cc.grid((5, 7), (2, 3), 4), cc.grid((70001,), (600,), 8, wrap=WRAP_GZIP), cc.grid((1,), (1,), 1)):
        for f in fc.all_filters():
            assert chunks_filters_bound(g, f) == chunks_bound(g) + 4 * f["fletcher32"] * cc.n_chunks(g)
    g3 = cc.grid((5,), (2,), 3)
    assert chunks_filters_bound(g3, fc.filters(fletcher32=1)) == chunks_bound(g3) + 12
    with pytest.raises(ValueError):  # (2^62 chunks of a byte: the grid is legal, the bound leaves int64)
        chunks_filters_bound(cc.grid((1 << 62,), (1,), 1), fc.NONE)
    L = _native.lib()
    assert L.zs_chunks_filters_bound(None, None) == -1 and L.zs_chunks_filters_bound(ctypes.byref(_native.ChunkGrid()), None) == -1


@pytest.mark.parametrize("good,bad", [
    ((2, dict(delta=1)), (3, dict(delta=1))), ((4, dict(delta=1)), (5, dict(delta=1))), ((8, dict(delta=1)), (16, dict(delta=1))),
    ((8, dict(byte_order=1)), (16, dict(byte_order=1))), ((2, dict(byte_order=1)), (3, dict(byte_order=1))), ((1, dict(byte_order=1, delta=1)), (7, dict(byte_order=1, delta=1))),
    ((3, dict(fletcher32=1)), (3, dict(fletcher32=1, reserved=1))), ((4, dict()), (4, dict(reserved=-1))),
    ((4, dict(delta=1)), (4, dict(delta=2))), ((4, dict(delta=0)), (4, dict(delta=-1))),
    ((4, dict(byte_order=1)), (4, dict(byte_order=2))), ((4, dict(byte_order=0)), (4, dict(byte_order=-1))),
    ((4, dict(fletcher32=1)), (4, dict(fletcher32=2))), ((4, dict(fletcher32=0)), (4, dict(fletcher32=-1))),
])
def test_each_filter_rule_from_both_sides(good, bad):
    """A rejected pair is ValueError (ZS_STREAM_ERROR from the grid check) in the bound and in both array calls, before any
    device work; its legal neighbour has a bound."""
    es, f = good
    assert chunks_filters_bound(cc.grid((5, 7), (2, 3), es), f) > 0
    es, f = bad
    g = cc.grid((5, 7), (2, 3), es)
    with pytest.raises(ValueError):
        chunks_filters_bound(g, f)
    with pytest.raises(ValueError):
        chunks_decode(None, [g], [[b"x"] * 6], [0x2000], [1 << 20], filters=[f])
    with pytest.raises(ValueError):
        chunks_encode(None, [g], [0x1000], [0x2000], [1 << 20], filters=[f])


def test_argument_checks_before_device_work():
    g = cc.grid((5, 7), (2, 3), 4)
    with pytest.raises(ValueError):
        chunks_decode(None, [g], [[b"x"] * 6], [0x2000], [1 << 20], filters=[])
    with pytest.raises(ValueError):
        chunks_decode(None, [g], [[b"x"] * 6], [0x2000], [1 << 20], filters=[{"delta": 1, "bitshuffle": 1}])
    with pytest.raises(ValueError):
        chunks_encode(None, [g], [0x1000], [0x2000], [1 << 20], filters=[fc.NONE, fc.NONE])
    for fn in (delta_encode, delta_decode):
        with pytest.raises(ValueError):
            fn(None, [0x1000], [0x2000], [8], [4])
        with pytest.raises(ValueError):
            fn(None, [0x1000], [0x2000], [8, 8], [4])
        assert fn(None, [], [], [], []) is None
    with pytest.raises(ValueError):
        fletcher32(None, [0x1000], [8])
    with pytest.raises(ValueError):
        fletcher32(None, [0x1000], [])
    assert fletcher32(None, [], []) == []
    L = _native.lib()
    VP = ctypes.c_void_p * 1
    assert L.zs_delta_encode_batch_device(None, 1, VP(0x1000), VP(0x2000), (ctypes.c_int64 * 1)(4), (ctypes.c_int * 1)(2), None) == ZS_STREAM_ERROR
    assert L.zs_fletcher32_batch_device(None, 1, VP(0x1000), (ctypes.c_int64 * 1)(4), (ctypes.c_uint32 * 1)(), None) == ZS_STREAM_ERROR
    assert L.zs_chunks_decode_filters_batch(None, 0, None, None, None, None, None, None, None, None) == ZS_STREAM_ERROR
    assert ctypes.sizeof(_native.ChunkFilters) == 16 and (FLETCHER32_TILE, DELTA_TILE) == (16384, 4096)


# ------------------------------------------------------------------ zarr_v2_filters
DELTA_I4 = {"id": "delta", "dtype": "<i4", "astype": "<i4"}
SHUFFLE4 = {"id": "shuffle", "elementsize": 4}
ACCEPTED = [
    (cc.zarray((10, 20), (4, 5)), dict(elem_size=4, shuffle=False, dtype="<f4"), fc.NONE),
    (cc.zarray((7,), (3,), dtype=">f4"), dict(elem_size=4, dtype=">f4"), fc.filters(byte_order=1)),
    (cc.zarray((7,), (3,), dtype=">f8", fill_value=1.5), dict(elem_size=8, fill=np.float64(1.5).tobytes()), fc.filters(byte_order=1)),
    (cc.zarray((7,), (3,), dtype=">i2", fill_value=-2, filters=[{"id": "shuffle", "elementsize": 2}]), dict(elem_size=2, shuffle=True, fill=np.int16(-2).tobytes()),
     fc.filters(byte_order=1)),
    (cc.zarray((7,), (3,), dtype=">i1"), dict(elem_size=1), fc.NONE),  # (a single byte has no order)
    (cc.zarray((7,), (3,), dtype="|u1", filters=[{"id": "delta", "dtype": "|u1", "astype": "|u1"}]), dict(elem_size=1), fc.filters(delta=1)),
    (cc.zarray((7,), (3,), dtype="<i4", filters=[DELTA_I4]), dict(elem_size=4, shuffle=False), fc.filters(delta=1)),
    (cc.zarray((7,), (3,), dtype="<i4", filters=[DELTA_I4, SHUFFLE4]), dict(elem_size=4, shuffle=True), fc.filters(delta=1)),
    (cc.zarray((7,), (3,), dtype="<i4", filters=[{"id": "delta", "dtype": "<i4"}]), dict(elem_size=4), fc.filters(delta=1)),  # (astype defaults to dtype)
    (cc.zarray((7,), (3,), dtype=">u8", filters=[{"id": "delta", "dtype": ">u8", "astype": ">u8"}, {"id": "shuffle", "elementsize": 8}], compressor={"id": "gzip", "level": 1}),
     dict(elem_size=8, shuffle=True, wrap=WRAP_GZIP, level=1), fc.filters(delta=1, byte_order=1)),
    (cc.zarray((7,), (3,), dtype="<c16"), dict(elem_size=16), fc.NONE),
]
REJECTED = [
    ("dtype", cc.zarray((7,), (3,), dtype=">c16"), cc.zarray((7,), (3,), dtype="<c16")),
    ("dtype", cc.zarray((7,), (3,), dtype=">U4"), cc.zarray((7,), (3,), dtype=">u4")),
    ("dtype", cc.zarray((7,), (3,), dtype=">q9"), cc.zarray((7,), (3,), dtype=">i8")),
    ("filters", cc.zarray((7,), (3,), dtype="<f4", filters=[{"id": "delta", "dtype": "<f4", "astype": "<f4"}]), cc.zarray((7,), (3,), dtype="<i4", filters=[DELTA_I4])),
    ("filters", cc.zarray((7,), (3,), dtype="<i4", filters=[{"id": "delta", "dtype": "<i4", "astype": "<i2"}]), cc.zarray((7,), (3,), dtype="<i4", filters=[DELTA_I4])),
    ("filters", cc.zarray((7,), (3,), dtype="<i4", filters=[{"id": "delta", "dtype": ">i4", "astype": ">i4"}]),
     cc.zarray((7,), (3,), dtype=">i4", filters=[{"id": "delta", "dtype": ">i4", "astype": ">i4"}])),
    ("filters", cc.zarray((7,), (3,), dtype="<i4", filters=[SHUFFLE4, DELTA_I4]), cc.zarray((7,), (3,), dtype="<i4", filters=[DELTA_I4, SHUFFLE4])),
    ("filters", cc.zarray((7,), (3,), dtype="<i4", filters=[DELTA_I4, DELTA_I4]), cc.zarray((7,), (3,), dtype="<i4", filters=[DELTA_I4])),
    ("filters", cc.zarray((7,), (3,), dtype="<i4", filters=[{"id": "fletcher32"}]), cc.zarray((7,), (3,), dtype="<i4", filters=[])),
    ("filters", cc.zarray((7,), (3,), dtype="<i4", filters=[{"id": "delta"}]), cc.zarray((7,), (3,), dtype="<i4", filters=[{"id": "delta", "dtype": "<i4"}])),
    ("order", cc.zarray((7,), (3,), dtype=">i4", order="F"), cc.zarray((7,), (3,), dtype=">i4")),
    ("zarr_format", cc.zarray((7,), (3,), dtype=">i4", zarr_format=3), cc.zarray((7,), (3,), dtype=">i4")),
    ("compressor", cc.zarray((7,), (3,), dtype=">i4", compressor={"id": "zstd", "level": 1}), cc.zarray((7,), (3,), dtype=">i4", compressor=None)),
]


@pytest.mark.parametrize("k", range(len(ACCEPTED)))
def test_zarr_v2_filters_accepts(k):
    doc, want, want_filters = ACCEPTED[k]
    for form in (doc, json.dumps(doc), json.dumps(doc).encode()):
        g, f = zarr_v2_filters(form)
        assert f == want_filters
        for key, v in want.items():
            assert g[key] == v, (key, g)
    assert chunks_filters_bound(g, f) == chunks_bound(g)  # (what it makes is a pair the library takes)
    if f == fc.NONE and g["elem_size"] > 1:
        assert g == zarr_v2_grid(doc)


@pytest.mark.parametrize("k", range(len(REJECTED)))
def test_zarr_v2_filters_rejects_naming_the_key(k):
    field, doc, neighbour = REJECTED[k]
    with pytest.raises(ValueError, match="zarr_v2_filters: %s:" % field):
        zarr_v2_filters(json.dumps(doc))
    zarr_v2_filters(json.dumps(neighbour))
