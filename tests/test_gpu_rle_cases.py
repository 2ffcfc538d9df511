"""CompressionStrategy.Rle over the chip (KR: zs_rle.hip's five launches, DeflateCall::rle_tiles, the hand-over to the tail
engine) on the inputs of tests/rle_cases.py, byte for byte against the oracle.  Why a case is here is its claim, which
tests/test_rle_cases.py holds against the oracle's stream on the CPU; here only bytes are compared, and a claim is never
evaluated on the device's stream.  Who ran a stream is asserted through zs_ctx_counter("lit_engine_bytes"): it grows by 0 for a
stream with rle_body_end(n) >= 0 and by n - 261 for one that is the literal engine's (tests/test_gpu_write_cases.py's convention).

The `measure` cases take deflate_batch_device from one torch buffer: its address is a multiple of 16 (asserted), every case lies
at an offset that is a multiple of 16 in it, and its slot start's position has the residue modulo 8 the case is named for -- so
the address the 8-byte loads of zs_rle_pass_kernel begin at has that residue."""
import io
import os
import zlib

import pytest

import rle_cases as rc
from test_rle_cases import ref
from zlibstream_amd import CompressionLevel, CompressionStrategy, ZlibOptions, ZlibOutputStream, deflate_bound

pytestmark = pytest.mark.gpu

SWITCHES = ("ZS_NO_RLE_RUNS", "ZS_NO_RLE_MULTI")
LEVELS = (1, 6, 9)
FF_STREAM = b"\xff" * 65537  # (tests/test_gpu_match_cases.py: the largest sums the trailer kernel combines)
SMALL = rc.small_names()
FAMILIES = sorted(f for f in rc.FAMILY_COUNTS if f not in ("pieces", "measure"))


@pytest.fixture(autouse=True)
def _clean_env():
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _lit(n, body=True):
    """what a stream of n bytes adds to lit_engine_bytes: nothing where the runs' kernels take the body"""
    return 0 if body and rc.body_end(n) >= 0 else max(0, n - 261)


def _counted(engine, call, **env):
    """(what `call` returns, what lit_engine_bytes grew by), under switches that are set for this call alone"""
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        before = engine.counter("lit_engine_bytes")
        out = call()
        return out, engine.counter("lit_engine_bytes") - before
    finally:
        for k in env:
            os.environ.pop(k, None)


def _device_writes(engine, datas, ends, level):
    """one zs_deflate_writes_batch_device call on fresh device buffers"""
    import torch
    d_in = [torch.frombuffer(bytearray(d) + bytearray(64), dtype=torch.uint8).cuda() for d in datas]
    caps = [deflate_bound(len(d)) for d in datas]
    d_out = [torch.full((c + 64,), 0xEE, dtype=torch.uint8, device="cuda") for c in caps]
    torch.cuda.synchronize()
    lens = engine.deflate_writes_batch_device([t.data_ptr() for t in d_in], [len(d) for d in datas], ends, [t.data_ptr() for t in d_out], caps, level=level,
                                              strategy=rc.RLE)
    return [bytes(t[:n].cpu().numpy()) for t, n in zip(d_out, lens)]


def test_the_catalogue_has_both_kinds_of_stream():
    sizes = [len(rc.case(n)[1]) for n in SMALL]
    assert len(SMALL) == 282 and sum(rc.body_end(n) < 0 for n in sizes) == 2 and min(sizes) == 4881


# ------------------------------------------------------------------ every case alone
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("family", FAMILIES)
def test_cases_alone(engine, oracle, family, level):
    bad = []
    for name in rc.case_names(family):
        data = rc.case(name)[1]
        (z,), lit = _counted(engine, lambda: engine.deflate_batch([data], level=level, strategy=rc.RLE))
        if z != ref(oracle, name, level) or lit != _lit(len(data)):
            bad.append((name, lit))
    assert not bad, bad


@pytest.mark.parametrize("name", rc.case_names("pieces"))
def test_pieces_case_alone(engine, oracle, name):
    """more than 1024 tiles: zs_rle_scan_kernel's `run` and zs_rle_sums_kernel's `total` go from piece to piece"""
    data = rc.case(name)[1]
    (z,), lit = _counted(engine, lambda: engine.deflate_batch([data], level=6, strategy=rc.RLE))
    assert lit == 0 and z == ref(oracle, name) and zlib.decompress(z) == data


@pytest.mark.parametrize("level", LEVELS)
def test_measure_cases_alone_at_their_addresses(engine, oracle, level):
    import torch
    names = rc.case_names("measure")
    offs, at = [], 0
    for n in names:
        offs.append(at)
        at += (len(rc.case(n)[1]) + 64 + 15) & ~15
    host = bytearray(at)
    for o, n in zip(offs, names):
        host[o:o + len(rc.case(n)[1])] = rc.case(n)[1]
    d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
    assert d_in.data_ptr() % 16 == 0
    seen, bad = set(), []
    out = torch.empty(deflate_bound(6000), dtype=torch.uint8, device="cuda")
    for o, n in zip(offs, names):
        p, r = rc.slot_start(n)
        assert (d_in.data_ptr() + o + p) % 8 == r
        seen.add((rc.AT[n][0], (d_in.data_ptr() + o + p) % 8))
        m = len(rc.case(n)[1])
        (k,), lit = _counted(engine, lambda: engine.deflate_batch_device([d_in.data_ptr() + o], [m], [out.data_ptr()], [out.numel()], level=level, strategy=rc.RLE,
                                                                       stream=torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        if out[:k].cpu().numpy().tobytes() != ref(oracle, n, level) or lit != 0:
            bad.append(n)
    assert len(seen) == len(rc.MEASURE_LEFT) * 8
    assert not bad, bad


# ------------------------------------------------------------------ in one batch
def _batch(order):
    names = SMALL[::-1] if order == "reversed" else SMALL
    return names, [rc.case(n)[1] for n in names] + [FF_STREAM]


@pytest.mark.parametrize("order", ["catalogue", "reversed"])
@pytest.mark.parametrize("level", LEVELS)
def test_cases_in_one_batch(engine, oracle, level, order):
    """rle_tile_off and blk_off are running sums over the streams; the two streams without a body stand between streams with
    one; an all-0xFF stream of 65 537 bytes among them, for the trailer"""
    names, bufs = _batch(order)
    got, lit = _counted(engine, lambda: engine.deflate_batch(bufs, level=level, strategy=rc.RLE))
    assert [n for n, z in zip(names, got) if z != ref(oracle, n, level)] == []
    assert got[-1] == oracle.compress(FF_STREAM, level, rc.RLE) and got[-1][-4:] == zlib.adler32(FF_STREAM).to_bytes(4, "big")
    assert lit == sum(_lit(len(b)) for b in bufs) == 2 * (4881 - 261)


def test_the_two_largest_pieces_cases_in_one_batch_with_three_small_ones(engine, oracle):
    big = sorted(rc.case_names("pieces"), key=lambda n: len(rc.case(n)[1]))[-2:]
    names = [big[0], "slot_run_775", "handover_n4881_filler", "handover_t1+257_run", big[1]]
    bufs = [rc.case(n)[1] for n in names]
    got, lit = _counted(engine, lambda: engine.deflate_batch(bufs, level=6, strategy=rc.RLE))
    assert [n for n, z in zip(names, got) if z != ref(oracle, n)] == []
    assert lit == 4881 - 261


@pytest.mark.parametrize("order", ["catalogue", "reversed"])
def test_cases_in_one_batch_on_the_literal_engine(engine, oracle, order):
    """ZS_NO_RLE_RUNS=1: a wave a stream, every stream whole (the pieces stay out: seconds per MiB there)"""
    names, bufs = _batch(order)
    got, lit = _counted(engine, lambda: engine.deflate_batch(bufs, level=6, strategy=rc.RLE), ZS_NO_RLE_RUNS=1)
    assert [n for n, z in zip(names, got) if z != ref(oracle, n)] == []
    assert got[-1] == oracle.compress(FF_STREAM, 6, rc.RLE)
    assert lit == sum(_lit(len(b), body=False) for b in bufs)


# ------------------------------------------------------------------ two Writes
_TWO = {}


def _two_ref(oracle, name, level):
    if (name, level) not in _TWO:
        _TWO[(name, level)] = oracle.compress(rc.case(name)[1], level, rc.RLE, chunks=rc.two_writes(name))
    return _TWO[(name, level)]


def _two_batch():
    datas = [rc.case(n)[1] for n in SMALL]
    ends = [[rc.two_writes(n)[0], len(d)] for n, d in zip(SMALL, datas)]
    assert all(not (e[0] >= 65536 - 262 and e[0] % 32768 >= 32768 - 262) and 0 < e[0] < e[1] for e in ends)
    return datas, ends


@pytest.mark.parametrize("level", LEVELS)
def test_cases_as_two_writes_fold_into_one(engine, oracle, level):
    """zs_deflate_writes_batch_device, one call: the first Write ends at a seeded position that is not within 262 below a window
    end, so fold_rle_writes makes the list the single Write and the runs' kernels take the body"""
    datas, ends = _two_batch()
    got, lit = _counted(engine, lambda: _device_writes(engine, datas, ends, level))
    assert [n for n, z in zip(SMALL, got) if z != _two_ref(oracle, n, level)] == []
    assert lit == sum(_lit(len(d)) for d in datas)


def test_cases_as_two_writes_on_the_literal_engine(engine, oracle):
    """ZS_NO_RLE_MULTI=1: the lists are not folded"""
    datas, ends = _two_batch()
    got, lit = _counted(engine, lambda: _device_writes(engine, datas, ends, 6), ZS_NO_RLE_MULTI=1)
    assert [n for n, z in zip(SMALL, got) if z != _two_ref(oracle, n, 6)] == []
    assert lit == sum(_lit(len(d), body=False) for d in datas)


# ------------------------------------------------------------------ through the Stream API
def test_handover_cases_through_the_stream_classes(engine, oracle):
    """ZlibOutputStream under CompressionStrategy.Rle, one Write and Close"""
    bad = []
    for name in rc.case_names("handover"):
        data = rc.case(name)[1]
        out = io.BytesIO()

        def call():
            s = ZlibOutputStream(out, ZlibOptions(CompressionLevel=CompressionLevel(6), CompressionStrategy=CompressionStrategy(rc.RLE)), engine=engine)
            s.write(data)
            s.close()
        _, lit = _counted(engine, call)
        if out.getvalue() != ref(oracle, name) or lit != _lit(len(data)):
            bad.append((name, lit))
    assert not bad, bad
