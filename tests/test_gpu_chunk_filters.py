"""The chunk filters on the device (include/zsgpu.h zs_chunk_filters): Fletcher-32, delta and big-endian elements, alone
(zs_fletcher32_batch_device, zs_delta_*_batch_device) and in the array calls (zs_chunks_*_filters_*).  Ground truth is
tests/chunk_filter_cases.py: the literal loop of H5_checksum_fletcher32 and the numpy model of the filter chain, written from the
header's rules.  Arrays are KiB-sized; every output lies between guard bytes at a chosen address modulo 16, pre-filled with a
sentinel."""
import struct

import numpy as np
import pytest

import chunk_cases as cc
import chunk_filter_cases as fc
from chunk_cases import ABSENT, SKIP, STORED, UNSHUFFLED, WRAP_GZIP, WRAP_RAW, WRAP_ZLIB, ZS_DATA_ERROR
from test_gpu_chunks import SENT, Arena, reference_streams
from zlibstream_amd import (DELTA_TILE, FLETCHER32_TILE, chunks_bound, chunks_decode, chunks_encode, chunks_filters_bound, delta_decode, delta_encode, fletcher32)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ zs_fletcher32_batch_device against the loop
def fletcher_on_device(engine, blobs, mods=None):
    a = Arena([len(b) for b in blobs], mods)
    for k, b in enumerate(blobs):
        a.put(k, b)
    got = fletcher32(engine, [a.ptr(k) for k in range(len(blobs))], [len(b) for b in blobs])
    a.results()  # (nothing but the inputs was written)
    return got


FLETCHER_LENGTHS = (0, 1, 2, 3, FLETCHER32_TILE - 1, FLETCHER32_TILE, FLETCHER32_TILE + 1, 2 * FLETCHER32_TILE + 1, 720, 721)


def test_fletcher32_lengths_and_addresses(engine):
    """Random, all-zero and all-0xff bytes at every edge length, the source at offsets 0..15 from a 16-byte boundary, all in one
    call."""
    rng = np.random.default_rng(2100)
    blobs, mods = [], []
    for k, n in enumerate(FLETCHER_LENGTHS):
        for kind in range(3):
            blobs.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes() if kind == 0 else bytes(n) if kind == 1 else b"\xff" * n)
            mods.append((5 * k + 7 * kind) % 16)
    for mod in range(16):  # every address, a length that ends mid-word and one of a tile and a half
        for n in (1003, FLETCHER32_TILE + FLETCHER32_TILE // 2 + 1):
            blobs.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
            mods.append(mod)
    got = fletcher_on_device(engine, blobs, mods)
    for b, m, v in zip(blobs, mods, got):
        assert v == fc.fletcher32_loop(b), (len(b), m, hex(v))


@pytest.mark.parametrize("n", FLETCHER_LENGTHS)
def test_fletcher32_one_span_a_call(engine, n):
    blob = np.random.default_rng(2200 + n).integers(0, 256, n, dtype=np.uint8).tobytes()
    assert fletcher_on_device(engine, [blob]) == [fc.fletcher32_loop(blob)]


def test_fletcher32_eight_mib(engine):
    """One span of 8 MiB: 512 tiles, folded by eight rounds of the wave."""
    blob = np.random.default_rng(2300).integers(0, 256, 8 << 20, dtype=np.uint8).tobytes()
    want = fc.fletcher32_loop(blob)
    assert want == fc.fletcher32_fast(blob)
    assert fletcher_on_device(engine, [blob], [9]) == [want]


# ------------------------------------------------------------------ the delta calls against the model
def delta_on_device(engine, fn, blobs, sizes, mods=None):
    src, dst = Arena([len(b) for b in blobs], mods), Arena([len(b) for b in blobs], mods)
    for k, b in enumerate(blobs):
        src.put(k, b)
    fn(engine, [src.ptr(k) for k in range(len(blobs))], [dst.ptr(k) for k in range(len(blobs))], [len(b) for b in blobs], sizes)
    src.results()
    return dst.results()


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_delta_encode_and_decode(engine, es):
    """Element counts 0, 1, around a lane's unit, a pass and a tile, and 65 tiles and a bit (the scan of the tile sums takes two
    rounds of its wave); values that wrap; leftover bytes; odd addresses.  Encode and decode against the model, and decode of
    encode is the identity."""
    counts = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, DELTA_TILE - 1, DELTA_TILE, DELTA_TILE + 1, 3 * DELTA_TILE + 5, 65 * DELTA_TILE + 33]
    rng = np.random.default_rng(2400 + es)
    blobs = []
    for k, count in enumerate(counts):
        left = k % es  # (0 .. es - 1 leftover bytes)
        a = rng.integers(0, 256, count * es + left, dtype=np.uint8)
        if count >= 4:
            a[:es] = 0xFF  # 0xff.. followed by 1: the difference and the sum wrap
            a[es:2 * es] = 0
            a[es] = 1
        blobs.append(a.tobytes())
    blobs.append(b"\xff" * (es * 300))  # every sum wraps
    sizes = [es] * len(blobs)
    enc = delta_on_device(engine, delta_encode, blobs, sizes)
    for b, e in zip(blobs, enc):
        assert e == fc.delta_encode(b, es), (len(b), es)
    dec = delta_on_device(engine, delta_decode, blobs, sizes)
    for b, d in zip(blobs, dec):
        assert d == fc.delta_decode(b, es), (len(b), es)
    back = delta_on_device(engine, delta_decode, enc, sizes, mods=[(3 * k) % 16 for k in range(len(blobs))])
    assert back == blobs


def test_delta_mixed_sizes_in_one_call(engine):
    rng = np.random.default_rng(2500)
    sizes = [1, 8, 2, 4, 4, 1, 8, 2]
    blobs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (5, 8 * 4097 + 3, 2 * 70 + 1, 4 * 1025, 0, 0, 7, 1)]
    for fn, model in ((delta_encode, fc.delta_encode), (delta_decode, fc.delta_decode)):
        assert delta_on_device(engine, fn, blobs, sizes) == [model(b, es) for b, es in zip(blobs, sizes)]
    with pytest.raises(ValueError):
        delta_on_device(engine, delta_encode, [bytes(6)], [3])
    with pytest.raises(ValueError):
        delta_on_device(engine, delta_decode, [bytes(32)], [16])


# ------------------------------------------------------------------ the array calls
def decode(engine, grids, fs, chunk_lists, mods=None, use_filters=True):
    sizes = [cc.array_bytes(g) for g in grids]
    arena = Arena(sizes, mods)
    rc, codes, status = chunks_decode(engine, grids, chunk_lists, [arena.ptr(k) for k in range(len(grids))], sizes, filters=fs if use_filters else None)
    return rc, codes, status, arena.results()


def encode(engine, grids, fs, datas, level=6, use_filters=True, **options):
    src = Arena([cc.array_bytes(g) for g in grids])
    for k, d in enumerate(datas):
        src.put(k, d)
    caps = [chunks_filters_bound(g, f) for g, f in zip(grids, fs)]
    dst = Arena(caps)
    n = len(grids)
    rc, lens, tables, status = chunks_encode(engine, grids, [src.ptr(k) for k in range(n)], [dst.ptr(k) for k in range(n)], caps, level=level,
                                             filters=fs if use_filters else None, **options)
    src.results()
    outs = dst.results(written=[ln if st == 0 else 0 for ln, st in zip(lens, status)])
    return rc, lens, tables, status, outs


def catalogue(es, wrap):
    """edge_grids under every combination of the three filters, shuffle on and off: (grids, filters, arrays)"""
    grids, fs, datas = [], [], []
    for f in fc.all_filters():
        for shuffle in (True, False):
            for k, g in enumerate(cc.edge_grids(es, shuffle, wrap, fill=bytes(range(1, es + 1)))):
                grids.append(g), fs.append(f)
                datas.append(fc.ramp_array(g, 40 * es + k) if f["delta"] else cc.smooth_array(g, 40 * es + k))
    return grids, fs, datas


@pytest.mark.parametrize("wrap", [WRAP_ZLIB, WRAP_RAW, WRAP_GZIP])
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_decode_every_combination(engine, es, wrap):
    """Chunks built by the model (padding that is not fill: it is ignored), decoded in one call, equal to the arrays."""
    grids, fs, datas = catalogue(es, wrap)
    lists = [fc.encoded_chunks(d, g, f, pad=b"\x77" * es) for g, f, d in zip(grids, fs, datas)]
    rc, codes, status, outs = decode(engine, grids, fs, lists)
    assert rc == 0 and status == [0] * len(grids), (rc, engine.last_error())
    for i, (g, f, d, o) in enumerate(zip(grids, fs, datas, outs)):
        assert codes[i] == [0] * cc.n_chunks(g)
        assert o == d, (i, g, f)


@pytest.mark.parametrize("wrap", [WRAP_ZLIB, WRAP_RAW, WRAP_GZIP])
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_encode_every_combination(engine, es, wrap):
    """Arrays encoded in one call: every chunk decodes through the model to the array's chunk, its checksum is the loop's, and its
    compressed bytes are zs_deflate_wrap_batch_device's over the model's filtered chunk."""
    grids, fs, datas = catalogue(es, wrap)
    rc, lens, tables, status, outs = encode(engine, grids, fs, datas)
    assert rc == 0 and status == [0] * len(grids), (rc, engine.last_error())
    want = [(i, c, fc.filtered_chunk(datas[i], g, fs[i], c)) for i, g in enumerate(grids) for c in range(cc.n_chunks(g))]
    ref = reference_streams(engine, [w[2] for w in want], wrap, 6)
    for (i, c, blob), stream in zip(want, ref):
        off, ln, flags = tables[i][c]
        stored = outs[i][off:off + ln]
        assert flags == 0 and stored == fc.stored_bytes(stream, fs[i]), (i, c, grids[i], fs[i])
        assert fc.decoded_chunk(stored, grids[i], fs[i]) == cc.chunk_of(datas[i], grids[i], c, shuffled=False), (i, c, grids[i], fs[i])
    for i, (g, f) in enumerate(zip(grids, fs)):
        at = 0
        for off, ln, _ in tables[i]:
            assert off == at and ln > 4 * f["fletcher32"]
            at += ln
        assert at == lens[i] <= chunks_filters_bound(g, f)


def flag_case(es=4):
    g = cc.grid((7, 141), (4, 70), es, fill=bytes(range(1, es + 1)))
    data = fc.ramp_array(g, 2600)
    return g, data


@pytest.mark.parametrize("f", fc.all_filters()[1:], ids=lambda f: "d%db%df%d" % (f["delta"], f["byte_order"], f["fletcher32"]))
def test_decode_flags_missing_and_skipped(engine, f):
    """STORED (it still carries delta, and its checksum is over the stored bytes), UNSHUFFLED, both, a missing chunk (fill, in the
    array's little-endian form) and a skipped one, in one array; and an all-stored unshuffled one (Zarr with compressor null)."""
    g, data = flag_case()
    assert cc.n_chunks(g) == 6
    sh = [fc.filtered_chunk(data, g, f, c, shuffled=True) for c in range(6)]
    pl = [fc.filtered_chunk(data, g, f, c, shuffled=False) for c in range(6)]
    z = lambda b: fc.stored_bytes(cc.compress(b, WRAP_ZLIB), f)  # noqa: E731
    chunks = [z(sh[0]), (fc.stored_bytes(sh[1], f), STORED), (z(pl[2]), UNSHUFFLED), (fc.stored_bytes(pl[3], f), STORED | UNSHUFFLED), None, (z(sh[5]), SKIP)]
    g2 = {**g, "shuffle": False, "stored": True}
    rc, codes, status, outs = decode(engine, [g, g2], [f, f], [chunks, [fc.stored_bytes(b, f) for b in pl]])
    assert rc == 0 and status == [0, 0] and codes == [[0] * 6, [0] * 6], engine.last_error()
    dec = [cc.chunk_of(data, g, c, shuffled=False) for c in range(6)]
    dec[4], dec[5] = None, "skip"
    assert outs[0] == cc.place(dec, g, into=bytes([SENT]) * cc.array_bytes(g))
    assert outs[1] == data


@pytest.mark.parametrize("f", fc.all_filters()[1:], ids=lambda f: "d%db%df%d" % (f["delta"], f["byte_order"], f["fletcher32"]))
def test_encode_skip_fill_and_allow_stored(engine, f):
    """SKIP_FILL looks at the array, whatever the filters; ALLOW_STORED stores the filtered bytes of a chunk that does not
    shrink (random bytes; zeros, and a row of random bytes above a row of padding, do shrink), checksum behind them; and what
    the call writes, the decode call reads back."""
    es = 4
    g = cc.grid((5, 140), (2, 70), es, fill=b"\x01\x02\x03\x04")
    a = np.frombuffer(cc.random_array(g, 2700), np.uint8).copy().reshape(5, 140, es)
    fill = np.frombuffer(g["fill"], np.uint8)
    a[cc.region(g, 0)] = fill
    a[cc.region(g, 5)] = fill
    a[cc.region(g, 3)] = 0
    data = a.tobytes()
    rc, lens, tables, status, outs = encode(engine, [g], [f], [data], skip_fill=True, allow_stored=True)
    assert rc == 0 and [t[2] for t in tables[0]] == [ABSENT, STORED, STORED, 0, 0, ABSENT], (tables, engine.last_error())
    cb = cc.chunk_bytes(g)
    for c, (off, ln, flags) in enumerate(tables[0]):
        stored = outs[0][off:off + ln]
        if flags & ABSENT:
            assert ln == 0
            continue
        assert ln == cb + 4 * f["fletcher32"] if flags & STORED else ln < cb + 4 * f["fletcher32"]
        if flags & STORED:
            assert stored == fc.stored_bytes(fc.filtered_chunk(data, g, f, c), f)
        assert fc.decoded_chunk(stored, g, f, flags) == cc.chunk_of(data, g, c, shuffled=False)
    chunks = [None if fl & ABSENT else (outs[0][off:off + ln], fl & STORED) for off, ln, fl in tables[0]]
    rc, codes, status, back = decode(engine, [g], [f], [chunks])
    assert rc == 0 and back[0] == data


# ------------------------------------------------------------------ failures, each between two whole chunks
@pytest.mark.parametrize("wrap", [WRAP_ZLIB, WRAP_GZIP])
@pytest.mark.parametrize("delta", [0, 1])
def test_checksum_failures_stay_in_their_chunk(engine, wrap, delta):
    f = fc.filters(delta=delta, byte_order=1, fletcher32=1)
    g = cc.grid((3, 210), (3, 70), 4, wrap=wrap, fill=b"\x01\x02\x03\x04")
    g_ok = cc.grid((9,), (4,), 2, wrap=wrap)
    data, data_ok = fc.ramp_array(g, 2800), cc.random_array(g_ok, 2801)
    enc, enc_ok = fc.encoded_chunks(data, g, f), fc.encoded_chunks(data_ok, g_ok, f)
    sentinel = bytes([SENT]) * cc.array_bytes(g)
    variants = fc.failing_checksum_chunks(fc.filtered_chunk(data, g, f, 1), g)
    assert len(variants) == 9
    for name, blob, flags, code, message in variants:
        rc, codes, status, outs = decode(engine, [g_ok, g, g_ok], [f, f, f], [enc_ok, [enc[0], (blob, flags), enc[2]], enc_ok])
        assert (rc, status, codes[1]) == (code, [0, code, 0], [0, code, 0]), (name, rc, status, codes, engine.last_error())
        assert engine.last_error() == "array 1: chunk 1: " + message, (name, engine.last_error())
        dec = [cc.chunk_of(data, g, 0, shuffled=False), "skip", cc.chunk_of(data, g, 2, shuffled=False)]
        assert outs[1] == cc.place(dec, g, into=sentinel), name  # the failing region still the sentinel, the neighbours exact
        assert outs[0] == data_ok and outs[2] == data_ok, name
    # inflate's own failures keep their messages behind a right checksum: the chunk is handed on, and fails there
    for name, blob, flags, code, message in cc.failing_chunks(fc.filtered_chunk(data, g, f, 1), g):
        if flags & STORED:
            continue
        rc, codes, status, outs = decode(engine, [g], [f], [[enc[0], (fc.with_checksum(blob), flags), enc[2]]])
        assert (rc, codes[0]) == (code, [0, code, 0]) and engine.last_error() == "array 0: chunk 1: " + message, (name, engine.last_error())
        assert outs[0] == cc.place([cc.chunk_of(data, g, 0, shuffled=False), "skip", cc.chunk_of(data, g, 2, shuffled=False)], g, into=sentinel), name


# ------------------------------------------------------------------ all filters 0: the present calls
@pytest.mark.parametrize("es", [1, 2, 3, 4, 8, 16])
def test_no_filters_is_the_present_call(engine, es):
    grids = cc.edge_grids(es, fill=bytes(range(1, es + 1))) + cc.edge_grids(es, shuffle=False, wrap=WRAP_GZIP)
    datas = [cc.smooth_array(g, 2900 + k) for k, g in enumerate(grids)]
    fs = [fc.NONE] * len(grids)
    lists = [cc.encoded_chunks(d, g) for d, g in zip(datas, grids)]
    bad = cc.failing_chunks(cc.chunk_of(datas[3], grids[3], 1), grids[3])
    lists[3][1] = (bad[0][1], bad[0][2])
    lists[5][0] = (bad[-1][1], bad[-1][2])
    a = decode(engine, grids, fs, lists, use_filters=False)
    message = engine.last_error()
    b = decode(engine, grids, fs, lists)
    assert a == b and engine.last_error() == message and a[0] == ZS_DATA_ERROR and message.startswith("array 3: chunk 1: ")
    for options in ({}, {"skip_fill": True, "allow_stored": True}):
        a = encode(engine, grids, fs, datas, use_filters=False, **options)
        b = encode(engine, grids, fs, datas, **options)
        assert a == b and a[0] == 0
    assert [chunks_filters_bound(g, fc.NONE) for g in grids] == [chunks_bound(g) for g in grids]
