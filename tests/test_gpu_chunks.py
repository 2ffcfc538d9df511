"""Chunked arrays on the device, both directions (include/zsgpu.h zs_chunks_*, zs_shuffle_batch_device): the chunks of HDF5 /
NetCDF-4 datasets and Zarr v2 arrays.  Ground truth is the numpy model of tests/chunk_cases.py (numpy, zlib and gzip), written
from the rules in the header.  Arrays are KiB-sized but for one 1-D chunk of 70,001 elements; every output lies between guard
bytes at a chosen address modulo 16, pre-filled with a sentinel."""
import numpy as np
import pytest

import chunk_cases as cc
from chunk_cases import ABSENT, SKIP, STORED, UNSHUFFLED, WRAP_GZIP, WRAP_RAW, WRAP_ZLIB, ZS_BUF_ERROR, ZS_DATA_ERROR
from zlibstream_amd import chunk_grid_info, chunks_bound, chunks_decode, chunks_encode, deflate_wrap_batch_device, shuffle, unshuffle, wrap_bound

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, 0xEE


class Arena:
    """Device buffers between guard bytes, buffer k at an address that is mods[k] modulo 16 (default: odd ones): ptr(k) is its
    address, put() uploads into it, results() returns every buffer's bytes and fails on a byte changed anywhere else."""

    def __init__(self, sizes, mods=None):
        import torch
        self.sizes = list(sizes)
        self.buf = torch.full((sum(self.sizes) + (GUARD + 32) * (len(self.sizes) + 1),), SENT, dtype=torch.uint8, device="cuda")
        base, at, self.off = self.buf.data_ptr(), GUARD, []
        for k, n in enumerate(self.sizes):
            want = (2 * k + 1) % 16 if mods is None else mods[k]
            at += (want - (base + at)) % 16
            self.off.append(at)
            at += n + GUARD
        torch.cuda.synchronize()

    def ptr(self, k):
        return self.buf.data_ptr() + self.off[k]

    def put(self, k, data):
        import torch
        a = np.frombuffer(bytes(data), np.uint8)
        if a.size:
            self.buf[self.off[k]:self.off[k] + a.size] = torch.from_numpy(a.copy()).cuda()

    def results(self, written=None):
        import torch
        torch.cuda.synchronize()
        got = self.buf.cpu().numpy()
        outside = got != SENT
        for k, (o, n) in enumerate(zip(self.off, self.sizes)):
            outside[o:o + (n if written is None else written[k])] = False
        assert not outside.any(), "bytes changed outside the outputs, first at %d" % int(np.flatnonzero(outside)[0])
        return [got[o:o + n].tobytes() for o, n in zip(self.off, self.sizes)]


def decode(engine, grids, chunk_lists, mods=None, caps=None):
    """chunks_decode into sentinel-filled buffers of exactly array_bytes (or caps[i]): (code, chunk codes, array codes, outputs)"""
    sizes = [cc.array_bytes(g) for g in grids]
    arena = Arena(sizes, mods)
    caps = sizes if caps is None else caps
    rc, codes, status = chunks_decode(engine, grids, chunk_lists, [arena.ptr(k) for k in range(len(grids))], caps)
    return rc, codes, status, arena.results()


def check_decode(engine, grids, datas, chunk_lists=None, mods=None):
    chunk_lists = [cc.encoded_chunks(d, g) for d, g in zip(datas, grids)] if chunk_lists is None else chunk_lists
    rc, codes, status, outs = decode(engine, grids, chunk_lists, mods)
    assert rc == 0 and status == [0] * len(grids), (rc, status, engine.last_error())
    for i, (g, d, o) in enumerate(zip(grids, datas, outs)):
        assert codes[i] == [0] * cc.n_chunks(g)
        assert o == d, "array %d %s: first difference at byte %d" % (i, g, next(k for k in range(len(d)) if o[k] != d[k]))


# ------------------------------------------------------------------ decode against place()
@pytest.mark.parametrize("es", [1, 2, 3, 4, 8, 16])
def test_decode_ranks_and_edges(engine, es):
    """Ranks 1..4, every axis 1 below, on and 1 above a chunk multiple: twelve arrays of different rank in one call."""
    grids = cc.edge_grids(es, fill=bytes(range(1, es + 1)))
    check_decode(engine, grids, [cc.random_array(g, 10 * es + k) for k, g in enumerate(grids)])


def test_decode_row_lengths(engine):
    """Last-axis chunk lengths giving rows of 1, 15, 16, 17 and 255 bytes, and the rows at which the lane unit changes (63, 64,
    511, 512 elements)."""
    rows = [(1, 1), (1, 15), (1, 16), (1, 17), (1, 255), (3, 5), (2, 8), (4, 4), (16, 1), (3, 85), (5, 51), (15, 17), (8, 2), (2, 63), (2, 64), (4, 511), (4, 512), (8, 513),
            (2, 600)]
    grids = [cc.grid((7, 2 * last + 1), (3, last), es) for es, last in rows]
    check_decode(engine, grids, [cc.random_array(g, 100 + k) for k, g in enumerate(grids)])


def test_decode_small_and_long(engine):
    """A one-element array, a chunk larger than the array, and one 1-D chunk of 70,001 elements of 4 bytes: its row spans
    several stretches and ends ragged."""
    grids = [cc.grid((1,), (1,), 4), cc.grid((1, 1, 1), (1, 1, 1), 3), cc.grid((3, 50), (8, 600), 4), cc.grid((5,), (4096,), 2), cc.grid((70001,), (70001,), 4),
             cc.grid((70001,), (70001,), 4, shuffle=False)]
    check_decode(engine, grids, [cc.smooth_array(g, 200 + k) for k, g in enumerate(grids)])


@pytest.mark.parametrize("es,chunks", [(4, (2, 520)), (2, (3, 70)), (8, (2, 16)), (1, (2, 520))])
def test_decode_output_alignment(engine, es, chunks):
    """out[i] at addresses 0..15 modulo 16, on every lane unit."""
    g = cc.grid(tuple(2 * c - 1 for c in chunks), chunks, es)
    datas = [cc.random_array(g, 300 + k) for k in range(16)]
    check_decode(engine, [g] * 16, datas, mods=list(range(16)))


def test_decode_wraps_and_shuffle(engine):
    """Each of the three containers, shuffle on and off, in one call."""
    grids = [cc.grid((9, 131), (4, 70), 4, shuffle=sh, wrap=w) for w in (WRAP_ZLIB, WRAP_RAW, WRAP_GZIP) for sh in (True, False)]
    check_decode(engine, grids, [cc.smooth_array(g, 400 + k) for k, g in enumerate(grids)])


def test_decode_flags(engine):
    """STORED, UNSHUFFLED and both together, beside a chunk with neither; and a grid whose chunks are all stored."""
    g = cc.grid((7, 141), (4, 70), 4)
    data = cc.random_array(g, 500)
    n = cc.n_chunks(g)
    assert n == 6
    sh = [cc.chunk_of(data, g, c, shuffled=True) for c in range(n)]
    pl = [cc.chunk_of(data, g, c, shuffled=False, pad=b"\x77" * 4) for c in range(n)]  # (padding is ignored when reading)
    chunks = [cc.compress(sh[0], WRAP_ZLIB), (sh[1], STORED), (cc.compress(pl[2], WRAP_ZLIB), UNSHUFFLED), (pl[3], STORED | UNSHUFFLED), (sh[4], STORED),
              cc.compress(sh[5], WRAP_ZLIB, 1)]
    g2 = {**g, "shuffle": False, "stored": True}  # a Zarr array with compressor null
    check_decode(engine, [g, g2], [data, data], [chunks, pl])


def test_decode_missing_and_skipped(engine):
    """A missing chunk in the interior and at a corner reads as fill (not all-equal bytes); a skipped chunk's region keeps the
    sentinel, with or without bytes given."""
    for es, fill in ((4, b"\x01\x02\x03\x04"), (3, b"\x09\x08\x07"), (1, b"\x05")):
        g = cc.grid((8, 200), (3, 70), es, fill=fill)
        data = cc.random_array(g, 600 + es)
        enc = cc.encoded_chunks(data, g)
        assert cc.n_chunks(g) == 9
        chunks = list(enc)
        chunks[4] = None
        chunks[8] = (None, 0)
        chunks[2] = (None, SKIP)
        chunks[6] = (enc[6], SKIP)
        rc, codes, status, outs = decode(engine, [g], [chunks])
        assert rc == 0 and status == [0] and codes == [[0] * 9], engine.last_error()
        dec = [cc.chunk_of(data, g, c, shuffled=False) for c in range(9)]
        dec[4] = dec[8] = None
        dec[2] = dec[6] = "skip"
        assert outs[0] == cc.place(dec, g, into=bytes([SENT]) * cc.array_bytes(g))


def test_decode_nothing(engine):
    assert chunks_decode(engine, [], [], [], []) == (0, [], [])


def test_decode_refuses_before_device_work(engine):
    g = cc.grid((5, 7), (2, 3), 4)
    enc = cc.encoded_chunks(cc.random_array(g, 1), g)
    arena = Arena([cc.array_bytes(g)])
    for bad_g, bad_chunks, cap in (({**g, "elem_size": 0}, enc, 1 << 20), (g, [(enc[0], 16)] + enc[1:], 1 << 20), (g, enc, -1),
                                   (cc.grid((1 << 31,), (1 << 31,), 1), [b"x"], 1 << 20)):
        with pytest.raises(ValueError):
            chunks_decode(engine, [bad_g], [bad_chunks], [arena.ptr(0)], [cap])
    arena.results(written=[0])


# ------------------------------------------------------------------ failures, each between two whole chunks
@pytest.mark.parametrize("wrap", [WRAP_ZLIB, WRAP_GZIP, WRAP_RAW])
def test_decode_failures_stay_in_their_chunk(engine, wrap):
    g = cc.grid((3, 210), (3, 70), 4, wrap=wrap, fill=b"\x01\x02\x03\x04")
    g_ok = cc.grid((9,), (4,), 2, wrap=wrap)
    data, data_ok = cc.smooth_array(g, 700), cc.random_array(g_ok, 701)
    enc, enc_ok = cc.encoded_chunks(data, g), cc.encoded_chunks(data_ok, g_ok)
    sentinel = bytes([SENT]) * cc.array_bytes(g)
    variants = cc.failing_chunks(cc.chunk_of(data, g, 1), g)
    assert {v[0] for v in variants} >= {"corrupted body", "a stream of chunk_bytes - elem_size", "a stream of chunk_bytes + elem_size", "a STORED chunk one byte short",
                                        "a stream cut in half"}
    for name, blob, flags, code, message in variants:
        chunks = [enc[0], (blob, flags), enc[2]]
        rc, codes, status, outs = decode(engine, [g_ok, g, g_ok], [enc_ok, chunks, enc_ok])
        assert (rc, status, codes[1]) == (code, [0, code, 0], [0, code, 0]), (name, rc, status, codes, engine.last_error())
        assert engine.last_error() == "array 1: chunk 1: " + message, (name, engine.last_error())
        dec = [cc.chunk_of(data, g, 0, shuffled=False), "skip", cc.chunk_of(data, g, 2, shuffled=False)]
        assert outs[1] == cc.place(dec, g, into=sentinel), name  # the failing region still the sentinel, the neighbours exact
        assert outs[0] == data_ok and outs[2] == data_ok, name
    # two failures in one array and one in the next: every code is there, the first one is named
    bad = {v[0]: v for v in variants}
    a, b = bad["a stream cut in half"], bad["a STORED chunk one byte short"]
    rc, codes, status, outs = decode(engine, [g, g], [[(b[1], b[2]), enc[1], (a[1], a[2])], [enc[0], (a[1], a[2]), enc[2]]])
    assert (rc, status, codes) == (ZS_DATA_ERROR, [ZS_DATA_ERROR, ZS_BUF_ERROR], [[ZS_DATA_ERROR, 0, ZS_BUF_ERROR], [0, ZS_BUF_ERROR, 0]])
    assert engine.last_error() == "array 0: chunk 0: incorrect chunk length"
    assert outs[0] == cc.place(["skip", cc.chunk_of(data, g, 1, shuffled=False), "skip"], g, into=sentinel)


def test_decode_short_capacity(engine):
    """An array with too little room is ZS_BUF_ERROR and nothing is written for it; the other one is complete."""
    g = cc.grid((7, 141), (4, 70), 4)
    data = cc.random_array(g, 800)
    enc = cc.encoded_chunks(data, g)
    n = cc.array_bytes(g)
    rc, codes, status, outs = decode(engine, [g, g], [enc, enc], caps=[n - 1, n])
    assert (rc, status, codes[0]) == (ZS_BUF_ERROR, [ZS_BUF_ERROR, 0], []) and engine.last_error() == "array 0: buffer error"
    assert outs[0] == bytes([SENT]) * n and outs[1] == data


# ------------------------------------------------------------------ encode
def encode(engine, grids, datas, level=6, caps=None, **options):
    """chunks_encode from arrays at odd addresses into sentinel-filled buffers: (code, lengths, chunk tables, codes, outputs)"""
    src = Arena([cc.array_bytes(g) for g in grids])
    for k, d in enumerate(datas):
        src.put(k, d)
    caps = [chunks_bound(g) for g in grids] if caps is None else caps
    dst = Arena(caps)
    n = len(grids)
    rc, lens, tables, status = chunks_encode(engine, grids, [src.ptr(k) for k in range(n)], [dst.ptr(k) for k in range(n)], caps, level=level, **options)
    src.results()
    outs = dst.results(written=[ln if st == 0 else 0 for ln, st in zip(lens, status)])
    return rc, lens, tables, status, outs


def reference_streams(engine, blobs, wrap, level):
    """zs_deflate_wrap_batch_device over these bytes"""
    src, dst = Arena([len(b) for b in blobs]), Arena([wrap_bound(len(b), wrap) for b in blobs])
    for k, b in enumerate(blobs):
        src.put(k, b)
    n = len(blobs)
    rc, lens, status = deflate_wrap_batch_device(engine, [src.ptr(k) for k in range(n)], [len(b) for b in blobs], [dst.ptr(k) for k in range(n)], dst.sizes, wrap, level=level)
    assert rc == 0
    return [o[:ln] for o, ln in zip(dst.results(), lens)]


def encode_grids():
    return [cc.grid((9, 131), (4, 70), 4, fill=b"\x01\x02\x03\x04"), cc.grid((5, 7, 19), (2, 3, 9), 3, fill=b"abc"), cc.grid((1201,), (600,), 8, wrap=WRAP_GZIP),
            cc.grid((4, 9, 3, 15), (2, 3, 2, 7), 2, wrap=WRAP_RAW), cc.grid((7, 141), (4, 70), 4, shuffle=False), cc.grid((1,), (1,), 16), cc.grid((33,), (16,), 1),
            cc.grid((3, 143), (2, 72), 4, fill=b"wxyz"), cc.grid((2, 1215), (1, 608), 2, fill=b"\x10\x20")]  # (rows one element short of a whole lane unit)


@pytest.mark.parametrize("level", [1, 6, 9])
def test_encode_streams(engine, level):
    """Every stream decodes through Python's zlib / gzip and the model's unshuffle to chunk_of(); offsets are back to back; the
    streams are, bit for bit, zs_deflate_wrap_batch_device's over the model's chunk bytes."""
    grids = encode_grids()
    datas = [cc.smooth_array(g, 900 + k) for k, g in enumerate(grids)]
    rc, lens, tables, status, outs = encode(engine, grids, datas, level=level)
    assert rc == 0 and status == [0] * len(grids), engine.last_error()
    for wrap in (WRAP_ZLIB, WRAP_RAW, WRAP_GZIP):
        want = [(i, c, cc.chunk_of(datas[i], g, c)) for i, g in enumerate(grids) if g["wrap"] == wrap for c in range(cc.n_chunks(g))]
        ref = reference_streams(engine, [w[2] for w in want], wrap, level)
        for (i, c, raw), stream in zip(want, ref):
            off, ln, flags = tables[i][c]
            assert flags == 0 and outs[i][off:off + ln] == stream, (i, c)
            assert cc.decompress(stream, wrap) == (raw, 0)
            assert cc.unshuffle(raw, grids[i]["elem_size"]) == cc.chunk_of(datas[i], grids[i], c, shuffled=False) or not grids[i]["shuffle"]
    for i, g in enumerate(grids):
        at = 0
        for off, ln, _ in tables[i]:
            assert off == at and ln > 0
            at += ln
        assert at == lens[i] <= chunks_bound(g)


def skip_fill_case():
    g = cc.grid((5, 140), (2, 70), 4, fill=b"\x01\x02\x03\x04")
    a = np.frombuffer(cc.random_array(g, 1000), np.uint8).copy().reshape(5, 140, 4)
    fill = np.frombuffer(g["fill"], np.uint8)
    a[cc.region(g, 0)] = fill  # all fill
    a[cc.region(g, 1)] = fill  # the same but for one byte of one element
    a[1, 139, 2] ^= 0x80
    a[cc.region(g, 5)] = fill  # an edge chunk: one row exists, and it is fill
    return g, a.tobytes()


def test_encode_skip_fill(engine):
    g, data = skip_fill_case()
    rc, lens, tables, status, outs = encode(engine, [g], [data], skip_fill=True)
    assert rc == 0 and [t[2] for t in tables[0]] == [ABSENT, 0, 0, 0, 0, ABSENT], tables
    assert [t[1] == 0 for t in tables[0]] == [True, False, False, False, False, True]
    at = 0
    for c, (off, ln, flags) in enumerate(tables[0]):
        assert off == at
        at += ln
        if not flags:
            assert cc.decompress(outs[0][off:off + ln], WRAP_ZLIB) == (cc.chunk_of(data, g, c), 0)
    # without the option every chunk is written
    rc, lens, tables, status, outs = encode(engine, [g], [data])
    assert rc == 0 and all(t[1] > 0 and t[2] == 0 for t in tables[0])
    assert cc.decompress(outs[0][:tables[0][0][1]], WRAP_ZLIB) == (cc.chunk_of(data, g, 0), 0)


def stored_case():
    g = cc.grid((4, 140), (2, 70), 4)
    a = np.frombuffer(cc.random_array(g, 1100), np.uint8).copy().reshape(4, 140, 4)
    a[cc.region(g, 1)] = 0
    a[cc.region(g, 2)] = 0
    return g, a.tobytes()


def test_encode_allow_stored(engine):
    """Random bytes are stored and zeros are compressed; without the option both are streams."""
    g, data = stored_case()
    cb = cc.chunk_bytes(g)
    rc, lens, tables, status, outs = encode(engine, [g], [data], allow_stored=True)
    assert rc == 0 and [t[2] for t in tables[0]] == [STORED, 0, 0, STORED]
    for c, (off, ln, flags) in enumerate(tables[0]):
        blob = outs[0][off:off + ln]
        assert (blob if flags else cc.decompress(blob, WRAP_ZLIB)[0]) == cc.chunk_of(data, g, c) and (ln == cb if flags else ln < cb)
    rc, lens, tables, status, outs = encode(engine, [g], [data])
    assert rc == 0 and [t[2] for t in tables[0]] == [0, 0, 0, 0] and tables[0][0][1] >= cb > tables[0][1][1]
    for c, (off, ln, flags) in enumerate(tables[0]):
        assert cc.decompress(outs[0][off:off + ln], WRAP_ZLIB) == (cc.chunk_of(data, g, c), 0)


def test_encode_short_capacity(engine):
    """A short out_cap reports the needed length and writes nothing; the other array is complete."""
    g = cc.grid((7, 141), (4, 70), 4)
    data = cc.smooth_array(g, 1200)
    rc, lens, tables, status, outs = encode(engine, [g, g], [data, data])
    assert rc == 0 and lens[0] == lens[1]
    need = lens[0]
    rc, lens2, tables2, status, outs2 = encode(engine, [g, g], [data, data], caps=[need - 1, need])
    assert (rc, status, lens2) == (ZS_BUF_ERROR, [ZS_BUF_ERROR, 0], [need, need]) and tables2 == tables
    assert outs2[0] == bytes([SENT]) * (need - 1) and outs2[1] == outs[1][:need]


def test_round_trip(engine):
    """What chunks_encode writes, chunks_decode reads back byte for byte: plain streams, skipped fill chunks, stored chunks."""
    grids = encode_grids()
    datas = [cc.smooth_array(g, 1300 + k) for k, g in enumerate(grids)]
    g1, d1 = skip_fill_case()
    g2, d2 = stored_case()
    grids, datas = grids + [g1, g2], datas + [d1, d2]
    rc, lens, tables, status, outs = encode(engine, grids, datas, skip_fill=True, allow_stored=True)
    assert rc == 0
    flags_seen = {f for t in tables for _, _, f in t}
    assert flags_seen == {0, STORED, ABSENT}
    chunk_lists = [[None if f & ABSENT else (o[off:off + ln], f & STORED) for off, ln, f in t] for t, o in zip(tables, outs)]
    check_decode(engine, grids, datas, chunk_lists)


def test_profiling_shows_the_kernels(engine):
    """zs_ctx_stage_ms shows KN as "chunk_kn" behind a decode (whose last call is an inflate), an encode and a shuffle."""
    g = cc.grid((7, 141), (4, 70), 4)
    data = cc.smooth_array(g, 1500)
    engine.set_profiling(True)
    try:
        rc, lens, tables, status, outs = encode(engine, [g], [data])
        enc_stages = engine.stage_ms()
        check_decode(engine, [g], [data], [[outs[0][off:off + ln] for off, ln, _ in tables[0]]])
        dec_stages = engine.stage_ms()
        a = Arena([64, 64])
        shuffle(engine, [a.ptr(0)], [a.ptr(1)], [64], [4])
        sh_stages = engine.stage_ms()
    finally:
        engine.set_profiling(False)
    assert enc_stages.get("chunk_kn", 0) > 0 and enc_stages.get("crc32_frame", 0) > 0, enc_stages
    assert dec_stages.get("chunk_kn", 0) > 0, dec_stages
    assert sh_stages.get("chunk_kn", 0) > 0, sh_stages


# ------------------------------------------------------------------ the stand-alone shuffles
def test_shuffle_and_unshuffle(engine):
    """Lengths 0, 1, es - 1, es, es + 1, 4097 and 65,537 for elem_size 1, 2, 3, 4, 7, 8 and 16, at odd addresses; plus lengths
    at which the lane unit changes."""
    cases = [(n, es) for es in (1, 2, 3, 4, 7, 8, 16) for n in (0, 1, es - 1, es, es + 1, 4097, 65537)]
    cases += [(4 * 63, 4), (4 * 64 + 3, 4), (2 * 511 + 1, 2), (8 * 512, 8), (4 * 4097, 4)]
    rng = np.random.default_rng(1400)
    blobs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n, _ in cases]
    for fn, model in ((shuffle, cc.shuffle), (unshuffle, cc.unshuffle)):
        src, dst = Arena([len(b) for b in blobs]), Arena([len(b) for b in blobs])
        for k, b in enumerate(blobs):
            src.put(k, b)
        fn(engine, [src.ptr(k) for k in range(len(blobs))], [dst.ptr(k) for k in range(len(blobs))], [len(b) for b in blobs], [es for _, es in cases])
        src.results()
        for (n, es), b, got in zip(cases, blobs, dst.results()):
            assert got == model(b, es), (fn.__name__, n, es)
    with pytest.raises(ValueError):
        shuffle(engine, [src.ptr(0)], [dst.ptr(0)], [8], [17])
    with pytest.raises(ValueError):
        unshuffle(engine, [src.ptr(0)], [dst.ptr(0)], [-1], [4])
