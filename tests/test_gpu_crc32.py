"""CRC-32 on the device (zs_crc32_device, zs_crc32_batch_device; KC, zs_crc32.hip) against Python's zlib.crc32, every comparison
exact.  Spans are carved from one random tensor at every start offset 0..15 behind a 256-byte boundary and at the lengths where
the kernel changes its path: 0..130 (no whole 16-byte word, one, several, the head and the tail in one word), one tile of T bytes
less, exactly and more than full, two tiles and a byte, and W tiles -- what one workgroup takes in a pass -- less and plus one
byte, where the fold crosses workgroups; one span of 3 MiB + 5 for the long exponents.  Zeros and 0xFF at the same lengths show a
wrong fold exponent that random data would also show, but without a second unknown."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = 3 * (1 << 20) + 5
POOL = BIG + 4096 + 256


def _tile_lengths():
    from zlibstream_amd.api import CRC32_TILE as T, CRC32_TILES_PER_WG as W
    return [T - 1, T, T + 1, 2 * T + 1, W * T - 1, W * T + 1]


@pytest.fixture(scope="module")
def pools():
    """name -> (host bytes, device tensor whose storage begins on a 256-byte boundary), made once and never written"""
    import torch
    rng = np.random.default_rng(3201)
    out = {}
    for name, host in (("random", rng.integers(0, 256, POOL, dtype=np.uint8)), ("zeros", np.zeros(POOL, dtype=np.uint8)),
                       ("ones", np.full(POOL, 0xFF, dtype=np.uint8))):
        dev = torch.from_numpy(host).cuda()
        assert dev.data_ptr() % 256 == 0
        out[name] = (host.tobytes(), dev)
    torch.cuda.synchronize()
    return out


def _spans(lengths):
    """(start, length) for every length at every offset 0..15 behind a 256-byte boundary, the boundaries spread over the pool"""
    out, k = [], 0
    for ln in lengths:
        for off in range(16):
            room = (POOL - ln - 16) // 256
            out.append((256 * (k * 7 % max(room, 1)) + off, ln))
            k += 1
    return out


def _check(engine, pool, spans, seeds=None, stream=None):
    from zlibstream_amd import crc32_batch_device
    host, dev = pool
    base = dev.data_ptr()
    got = crc32_batch_device(engine, [base + s for s, _ in spans], [n for _, n in spans], seeds, stream=stream)
    want = [zlib.crc32(host[s:s + n], seeds[i] if seeds else 0) for i, (s, n) in enumerate(spans)]
    bad = [(spans[i], hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("data", ["random", "zeros", "ones"])
def test_every_length_to_130_at_every_offset(engine, pools, data):
    _check(engine, pools[data], _spans(range(131)))


@pytest.mark.parametrize("data", ["random", "zeros", "ones"])
def test_tile_edges_and_the_fold_across_workgroups(engine, pools, data):
    _check(engine, pools[data], _spans(_tile_lengths()))


@pytest.mark.parametrize("data", ["random", "zeros", "ones"])
def test_three_mib_and_five_at_every_offset(engine, pools, data):
    _check(engine, pools[data], [(off, BIG) for off in range(16)])


@pytest.mark.parametrize("seed", [0, 0xFFFFFFFF, zlib.crc32(b"IDAT")])
def test_seeds(engine, pools, seed):
    spans = _spans(list(range(0, 40)) + _tile_lengths())[::3] + [(5, BIG)]
    _check(engine, pools["random"], spans, [seed] * len(spans))
    _check(engine, pools["zeros"], spans, [seed] * len(spans))


def test_mixed_batch_keeps_input_order(engine, pools):
    from zlibstream_amd.api import CRC32_TILE as T
    lens = [0, 1, BIG, 0, 17, 5 * T + 3, 2, 0, 1 << 20, 3, T, 0]
    spans = [(3 + 256 * i + i, n) for i, n in enumerate(lens)]
    _check(engine, pools["random"], spans, [(0x9E3779B9 * i) & 0xFFFFFFFF for i in range(len(lens))])


def test_empty_calls_and_null_pointers_of_empty_spans(engine):
    from zlibstream_amd import crc32_batch_device, crc32_device
    assert crc32_batch_device(engine, [], []) == []
    assert crc32_batch_device(engine, [0, 0], [0, 0], [0, 0x12345678]) == [0, 0x12345678]
    assert crc32_device(engine, 0, 0, seed=77) == 77


def test_on_a_stream_of_the_caller(engine, pools):
    import torch
    s = torch.cuda.Stream()
    _check(engine, pools["random"], _spans(_tile_lengths() + [0, 1, 100]), stream=s.cuda_stream)
    s.synchronize()


def test_single_span_call_continued_over_three_pieces(engine, pools):
    from zlibstream_amd import crc32_device
    from zlibstream_amd.api import CRC32_TILE as T
    host, dev = pools["random"]
    for start, cuts in ((0, (0, 0, 9)), (7, (1, T, 2 * T + 11)), (13, (100003, 100003, BIG - 13)), (1, (5, 6, 7))):
        a, b, c = cuts
        pieces = ((start, a), (start + a, b - a), (start + b, c - b))
        crc = 0
        for s, n in pieces:
            crc = crc32_device(engine, dev.data_ptr() + s, n, seed=crc)
        assert crc == zlib.crc32(host[start:start + c]), (start, cuts)
        assert crc32_device(engine, dev.data_ptr() + start, c) == crc


def test_bad_arguments_are_stream_errors_before_any_device_work(engine, pools):
    import ctypes
    from zlibstream_amd import _native, crc32_batch_device, crc32_device
    L = _native.lib()
    _, dev = pools["random"]
    p = dev.data_ptr()
    out = (ctypes.c_uint32 * 1)(0xABCD)
    VP, I64 = ctypes.c_void_p * 1, ctypes.c_int64 * 1
    assert L.zs_crc32_batch_device(None, 1, VP(p), I64(4), None, out, None) == -2
    assert L.zs_crc32_batch_device(engine.handle, -1, VP(p), I64(4), None, out, None) == -2
    assert L.zs_crc32_batch_device(engine.handle, 1, None, I64(4), None, out, None) == -2
    assert L.zs_crc32_batch_device(engine.handle, 1, VP(p), None, None, out, None) == -2
    assert L.zs_crc32_batch_device(engine.handle, 1, VP(p), I64(4), None, None, None) == -2
    assert L.zs_crc32_batch_device(engine.handle, 1, VP(p), I64(-1), None, out, None) == -2
    assert L.zs_crc32_batch_device(engine.handle, 1, VP(p), I64((1 << 31) - 1023), None, out, None) == -2
    assert L.zs_crc32_batch_device(engine.handle, 1, VP(None), I64(4), None, out, None) == -2
    assert L.zs_crc32_batch_device(engine.handle, 0, None, None, None, None, None) == 0
    assert out[0] == 0xABCD
    for bad in ((p, -1), (p, 1 << 31), (0, 5)):
        with pytest.raises(ValueError):
            crc32_device(engine, *bad)
        with pytest.raises(ValueError):
            crc32_batch_device(engine, [bad[0]], [bad[1]])
    with pytest.raises(ValueError):
        crc32_batch_device(engine, [p], [4, 4])
    with pytest.raises(ValueError):
        crc32_batch_device(engine, [p], [4], [1 << 32])


def test_the_stage_timer_shows_the_launch(engine, pools):
    from zlibstream_amd import crc32_device
    _, dev = pools["random"]
    engine.set_profiling(True)
    try:
        crc32_device(engine, dev.data_ptr(), BIG)
        stages = engine.stage_ms()
    finally:
        engine.set_profiling(False)
    assert stages.get("crc32_frame", 0) > 0, stages
