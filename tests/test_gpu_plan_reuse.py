"""A deflate call of the shape of the one before takes its plan (zlibstream_amd/csrc/zs_plan_key.h): the
host skips planning, the workspace walk, the geometry and work-list uploads and zs_worklist_kernel, and sends the descriptors
with the caller's pointers alone.  Every output is compared byte for byte with the oracle; zs_ctx_counter("plan_reused") says
whether a call took the kept plan.  Sizes: 1 MiB + 3 bytes of text at level 6 (the speculative walk), 70 000 bytes at level 6
(the maps), 300 000 bytes at level 1 (the sweeps), 64 KiB of sparse rows at level 6 (periodic data).

300 000 bytes at level 1 is planned for the sweeps and for the speculative runs at once, and the links decide in every call
(zs_plan.h plan_streams, allow_dual): the kept plan keeps both.  300 KiB of sparse rows at level 1 is the same plan with the other answer -- and its runs
do not verify, so the batch is run again on one run of the engine per stream (fast_fallbacks): a call that ends in a re-entry of
the pipeline ends on a plan that is never kept, and its counter is 0 every time."""
import io

import pytest

from zlibstream_amd import Engine, ZlibOptions, ZlibOutputStream, ZlibStreamException, FlushMode, datagen, deflate_bound
from zlibstream_amd.api import png_filter_batch_device, png_idat_batch_device

pytestmark = pytest.mark.gpu

GOLDEN = datagen.GOLDEN
SHAPES = {"walk": ((1 << 20) + 3, 6), "maps": (70000, 6), "sweeps": (300000, 1), "periodic": (64 << 10, 6), "runs": (307200, 1)}


@pytest.fixture(scope="module")
def texts():
    """two different buffers per shape (b is not a shifted a: other words from the first byte on)"""
    a = datagen.english((1 << 20) + 3)
    b = datagen.english((1 << 20) + 3, (GOLDEN + 17) & datagen.MASK)
    out = {k: (a[:n], b[:n]) for k, (n, _) in SHAPES.items() if k not in ("periodic", "runs")}
    out["periodic"] = (datagen.sparse(128, 128), datagen.sparse(128, 128, y0=77))
    out["runs"] = (datagen.sparse(256, 300), datagen.sparse(256, 300, y0=77))  # level 1: the links say "periodic"
    return out


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's bytes, computed once per (buffer, level, strategy, Writes)"""
    memo = {}

    def get(data, level, strategy=0, ends=None):
        key = (hash(data), len(data), level, strategy, tuple(ends) if ends else None)
        if key not in memo:
            sizes = [e - s for s, e in zip([0] + list(ends[:-1]), ends)] if ends else None
            memo[key] = oracle.compress(data, level, strategy, chunks=sizes if sizes and len(sizes) > 1 else None)
        return memo[key]

    return get


@pytest.fixture()
def eng():
    e = Engine(0)
    yield e
    e.close()


def _run(e, datas, level, strategy=0, ends=None, offset=0, caps=None):
    """One zs_deflate(_writes)_batch_device call on fresh device buffers, the inputs `offset` bytes into their allocations.
    Returns (streams, plan_reused)."""
    import torch
    d_in = [torch.frombuffer(bytearray(offset) + bytearray(d) + bytearray(64), dtype=torch.uint8).cuda() for d in datas]
    caps = caps or [deflate_bound(len(d)) for d in datas]
    d_out = [torch.full((c + 64,), 0xEE, dtype=torch.uint8, device="cuda") for c in caps]
    torch.cuda.synchronize()
    lens = e.deflate_writes_batch_device([t.data_ptr() + offset for t in d_in], [len(d) for d in datas], ends, [t.data_ptr() for t in d_out], caps,
                                         level=level, strategy=strategy)
    return [bytes(t[:n].cpu().numpy()) for t, n in zip(d_out, lens)], e.counter("plan_reused")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_same_shape_twice_other_data_other_pointers(eng, texts, want, shape):
    """The second and third call have the first's shape, other bytes and other device buffers, the third's input at an odd
    address: both take the kept plan, every output is the oracle's."""
    a, b = texts[shape]
    level = SHAPES[shape][1]
    (z,), r = _run(eng, [a], level)
    assert r == 0 and z == want(a, level)
    reused = 0 if shape == "runs" else 1
    (z,), r = _run(eng, [b], level)
    assert r == reused and z == want(b, level)
    (z,), r = _run(eng, [a], level, offset=3)
    assert r == reused and z == want(a, level)
    if shape == "walk":
        assert eng.counter("spec_streams") == 1 and eng.counter("spec_fallbacks") == 0
    if shape == "sweeps":
        assert eng.counter("fast_rounds") > 0
    if shape == "runs":
        assert eng.counter("fast_rounds") == 0 and eng.counter("fast_fallbacks") == 3  # (every call ran its batch again)


def test_same_lengths_other_level_strategy_or_writes_is_not_reused(eng, texts, want):
    a, b = texts["maps"]
    n = len(a)
    (z,), r = _run(eng, [a], 6)
    assert r == 0 and z == want(a, 6)
    (z,), r = _run(eng, [b], 5)
    assert r == 0 and z == want(b, 5)
    (z,), r = _run(eng, [b], 5)
    assert r == 1 and z == want(b, 5)
    (z,), r = _run(eng, [a], 5, strategy=1)
    assert r == 0 and z == want(a, 5, 1)
    (z,), r = _run(eng, [a], 5, strategy=1)
    assert r == 1 and z == want(a, 5, 1)
    ends = [100, 30000, n]
    (z,), r = _run(eng, [b], 5, strategy=1, ends=[ends])
    assert r == 0 and z == want(b, 5, 1, ends)
    (z,), r = _run(eng, [a], 5, strategy=1, ends=[ends])
    assert r == 1 and z == want(a, 5, 1, ends)
    other = [100, 30001, n]
    (z,), r = _run(eng, [a], 5, strategy=1, ends=[other])
    assert r == 0 and z == want(a, 5, 1, other)
    (z,), r = _run(eng, [b], 5, strategy=1)
    assert r == 0 and z == want(b, 5, 1)


def test_one_length_of_a_batch_changed_by_one_byte(eng, texts, want):
    a, b = texts["walk"]
    batch = [a[:70000], b[:40001], a[5:65541]]
    zs, r = _run(eng, batch, 6)
    assert r == 0 and zs == [want(d, 6) for d in batch]
    again = [b[:70000], a[:40001], b[5:65541]]
    zs, r = _run(eng, again, 6)
    assert r == 1 and zs == [want(d, 6) for d in again]
    longer = [a[:70000], b[:40002], a[5:65541]]
    zs, r = _run(eng, longer, 6)
    assert r == 0 and zs == [want(d, 6) for d in longer]
    zs, r = _run(eng, batch, 6)
    assert r == 0 and zs == [want(d, 6) for d in batch]


def test_other_calls_in_between(eng, texts, want):
    """An inflate call, PNG filter calls, a PNG IDAT call (a deflate of its own) and a Write-list call between same-shaped
    calls: the bytes are right whatever came in between, and the counter says who writes what the kept plan lives in.  Inflate
    checks its Adler-32 through the deflate pipeline's descriptors and work items (device_adlers): no plan is left.  The first
    PNG filter call of a context allocates its buffers, and any buffer that moves drops the plan; the second allocates nothing
    and has descriptors of its own: the plan stays."""
    import torch
    a, b = texts["maps"]
    (z,), r = _run(eng, [a], 6)
    assert r == 0 and z == want(a, 6)
    (z,), r = _run(eng, [b], 6)
    assert r == 1 and z == want(b, 6)
    assert eng.inflate_batch([want(b, 6)], [len(b)]) == [b]
    (z,), r = _run(eng, [b], 6)
    assert r == 0 and z == want(b, 6)
    assert eng.inflate_batch([want(a, 6)], [len(a)]) == [a]  # (nothing grows this time: it is the Adler call that counts)
    (z,), r = _run(eng, [a], 6)
    assert r == 0 and z == want(a, 6)
    px = datagen.sparse(64, 32)
    d_px = torch.frombuffer(bytearray(px) + bytearray(16), dtype=torch.uint8).cuda()
    d_f = torch.zeros(32 * 257 + 32, dtype=torch.uint8, device="cuda")
    d_z = torch.zeros(16384, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    png_filter_batch_device(eng, [d_px.data_ptr()], [256], [32], [4], [4], [d_f.data_ptr()])
    (z,), r = _run(eng, [b], 6)
    assert r == 0 and z == want(b, 6)
    png_filter_batch_device(eng, [d_px.data_ptr()], [256], [32], [4], [4], [d_f.data_ptr()])
    (z,), r = _run(eng, [a], 6)
    assert r == 1 and z == want(a, 6)
    png_idat_batch_device(eng, [d_px.data_ptr()], [256], [32], [4], [4], [d_z.data_ptr()], [16384])
    (z,), r = _run(eng, [b], 6)
    assert r == 0 and z == want(b, 6)  # (the IDAT call planned a deflate of its own)
    ends = [5, 69000, len(a)]
    (zw,), r = _run(eng, [a], 6, ends=[ends])
    assert r == 0 and zw == want(a, 6, 0, ends)
    (z,), r = _run(eng, [a], 6)
    assert r == 0 and z == want(a, 6)
    (z,), r = _run(eng, [b], 6)
    assert r == 1 and z == want(b, 6)


def test_the_live_block_list_and_its_switch(eng, want, monkeypatch):
    """64 streams and more: every call rewrites the block list of the work array with the blocks its streams have
    (zs_live_fill_kernel), unless ZS_NO_LIVE_LIST is set -- then it reads the list zs_worklist_kernel made.  A kept plan keeps
    the work array, so the switch is part of the key.  64 streams of 40 000 bytes: text is one block a stream, random bytes
    three, so a list left by a call on text lacks blocks that a call on random bytes has."""
    import numpy as np
    n, size = 64, 40000
    text = datagen.english(n * size, (GOLDEN + 5) & datagen.MASK)
    rnd = np.random.default_rng(99).integers(0, 256, n * size, dtype=np.uint8).tobytes()
    texts_, rnds = [text[i * size:(i + 1) * size] for i in range(n)], [rnd[i * size:(i + 1) * size] for i in range(n)]
    mixed = [rnds[i] if i % 3 == 0 else texts_[i] for i in range(n)]

    def check(datas, reused):
        zs, r = _run(eng, datas, 6)
        assert r == reused
        assert zs == [want(d, 6) for d in datas]

    check(texts_, 0)
    check(rnds, 1)        # the live list, rewritten by each call: more blocks than the call before
    check(mixed, 1)       # ... and fewer
    monkeypatch.setenv("ZS_NO_LIVE_LIST", "1")
    check(rnds, 0)        # the switch flipped: the list the call before left (one block of three) must not serve
    check(texts_, 1)      # the list as zs_worklist_kernel made it, kept
    check(mixed, 1)
    monkeypatch.delenv("ZS_NO_LIVE_LIST")
    check(rnds, 0)
    check(texts_, 1)


def test_a_call_that_grows_the_workspace_in_between(eng, texts, want):
    a, b = texts["walk"]
    small_a, small_b = texts["maps"]
    (z,), r = _run(eng, [small_a], 6)
    assert r == 0 and z == want(small_a, 6)
    (z,), r = _run(eng, [a], 6)
    assert r == 0 and z == want(a, 6)
    (z,), r = _run(eng, [small_b], 6)
    assert r == 0 and z == want(small_b, 6)
    (z,), r = _run(eng, [small_a], 6)
    assert r == 1 and z == want(small_a, 6)


def test_a_stream_of_eight_flushed_writes(texts, oracle):
    """The Stream API: eight Writes of 64 KiB, a Sync flush behind each, on one engine twice over -- the runs of an incremental
    stream plan afresh every time, between and beside calls that keep plans."""
    a, b = texts["walk"]
    e = Engine(0)
    try:
        for data in (a[:8 * 65536], b[:8 * 65536]):
            sink = io.BytesIO()
            s = ZlibOutputStream(sink, ZlibOptions(CompressionLevel=6, FlushMode=FlushMode.SyncFlush), engine=e)
            for k in range(8):
                s.write(data[k * 65536:(k + 1) * 65536])
                assert e.counter("plan_reused") == 0
            s.close()
            assert sink.getvalue() == oracle.compress_writes(data, 6, 0, [65536] * 8, [int(FlushMode.SyncFlush)] * 8)
    finally:
        e.close()


def test_a_call_that_fails_then_the_same_shape_with_room(eng, texts, want):
    a, b = texts["maps"]
    (z,), r = _run(eng, [a], 6)
    assert r == 0 and z == want(a, 6)
    with pytest.raises(ZlibStreamException):
        _run(eng, [b], 6, caps=[1000])
    assert eng.counter("plan_reused") == 0
    (z,), r = _run(eng, [b], 6)
    assert r == 0 and z == want(b, 6)
    with pytest.raises(ZlibStreamException):
        _run(eng, [a], 6, caps=[1000])
    with pytest.raises(ZlibStreamException):
        _run(eng, [b], 6, caps=[1000])
    assert eng.counter("plan_reused") == 1  # (a failing call's shape is a shape too)
    (z,), r = _run(eng, [a], 6)
    assert r == 0 and z == want(a, 6)


# (switch, value, the texts' shape, bytes of it, level, strategy, Write ends): the smallest shape on which the switch acts.  Every
# row changes the plan but ZS_FAST_CHUNK=65536, which is what 300 000 bytes get anyway: that row shows the key alone (the value
# counts as set); tests/cpp/test_plan.cpp takes 262144, which changes the runs
PLANNER_SWITCHES = [
    ("ZS_NO_SPEC", "1", "walk", None, 6, 0, None),
    ("ZS_SPEC_LEN", "512", "walk", None, 6, 0, None),
    ("ZS_SPEC_MIN", "2097152", "walk", None, 6, 0, None),
    ("ZS_NO_FAST_VEC", "1", "sweeps", None, 1, 0, None),
    ("ZS_FAST_NO_ROUNDS", "1", "sweeps", None, 1, 0, None),
    ("ZS_FR_RATIO", "0", "sweeps", None, 1, 0, None),
    ("ZS_FR_CHUNK", "4096", "sweeps", None, 1, 0, None),
    ("ZS_FAST_CHUNK", "65536", "sweeps", None, 1, 0, None),
    ("ZS_NO_RLE_RUNS", "1", "maps", 70000, 6, 3, None),
    ("ZS_NO_RLE_MULTI", "1", "maps", 70000, 6, 3, [30000, 70000]),
    ("ZS_NO_FAST_MULTI", "1", "sweeps", 300000, 1, 0, [81920, 163840, 245760, 300000]),
]


@pytest.mark.parametrize("switch,value,shape,size,level,strategy,ends", PLANNER_SWITCHES, ids=[c[0] for c in PLANNER_SWITCHES])
def test_a_planner_switch_flipped_between_same_shaped_calls(eng, texts, want, monkeypatch, switch, value, shape, size, level, strategy, ends):
    """Every switch the planner takes from the key's PlanEnv (zs_plan.h), on the smallest shape where it acts: buffer a, buffer b,
    the switch set, a, b, the switch unset, a.  A call under another setting plans afresh, the one behind it takes that plan:
    plan_reused reads 0, 1, 0, 1, 0, and every output is the oracle's.  ZS_NO_FAST_RESUME and ZS_NO_RESUME_ROUNDS act only on
    the runs of an incremental stream, whose plans are never kept: tests/cpp/test_plan.cpp has them, on the host."""
    a, b = (d[:size] if size else d for d in texts[shape])
    expect = {id(a): want(a, level, strategy, ends), id(b): want(b, level, strategy, ends)}

    def call(data, reused):
        (z,), r = _run(eng, [data], level, strategy=strategy, ends=[ends] if ends else None)
        assert r == reused and z == expect[id(data)]

    call(a, 0)
    call(b, 1)
    monkeypatch.setenv(switch, value)
    call(a, 0)
    call(b, 1)
    monkeypatch.delenv(switch)
    call(a, 0)


def test_the_switch_turns_reuse_off(eng, texts, want, monkeypatch):
    a, b = texts["maps"]
    monkeypatch.setenv("ZS_NO_PLAN_REUSE", "1")
    for d in (a, b, a):
        (z,), r = _run(eng, [d], 6)
        assert r == 0 and z == want(d, 6)
    monkeypatch.delenv("ZS_NO_PLAN_REUSE")
    (z,), r = _run(eng, [b], 6)
    assert r == 0 and z == want(b, 6)
    monkeypatch.setenv("ZS_NO_SPEC", "1")  # a switch the planning reads: the plan made without it does not serve
    (z,), r = _run(eng, [a], 6)
    assert r == 0 and z == want(a, 6)
    (z,), r = _run(eng, [b], 6)
    assert r == 1 and z == want(b, 6)
