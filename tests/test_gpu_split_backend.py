"""The split back end: with the tail engine on the second stream, the blocks that end inside the body go
through K5b, K7, K8 and K9 beside it (part 0) and only what the tail engine writes follows behind it (part 1).  Every case
runs as it is and with ZS_NO_SPLIT_BACKEND, which keeps the one-launch order; both are the oracle's bytes.  Streams of a few
hundred KiB at most; ZS_SPEC_MIN=65536 makes those from 64 KiB on take the speculative walk."""
import io
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import deflate_reader
import test_spec_model as model
from zlibstream_amd import CompressionLevel, CompressionStrategy, Engine, ZlibOptions, ZlibOutputStream, deflate_bound

pytestmark = pytest.mark.gpu

SWITCHES = ("ZS_NO_SPLIT_BACKEND", "ZS_SPEC_MIN", "ZS_SPEC_CORRUPT", "ZS_NO_SPEC", "ZS_NO_PLAN_REUSE")
BLOCK = 16383  # kBlockSyms
ZS_BUF_ERROR = -5


@pytest.fixture(autouse=True)
def _clean_env():
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _with_env(fn, **env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


def _both(fn, **env):
    """fn() with the back end split and with ZS_NO_SPLIT_BACKEND"""
    return _with_env(fn, **env), _with_env(fn, ZS_NO_SPLIT_BACKEND=1, **env)


def _check(engine, oracle, bufs, level=6, strategy=0, **env):
    split, whole = _both(lambda: engine.deflate_batch(bufs, level=level, strategy=strategy), **env)
    want = [oracle.compress(d, level, strategy) for d in bufs]
    bad = [(i, len(d)) for i, d in enumerate(bufs) if split[i] != want[i]]
    assert not bad, "split back end differs from the oracle: %r" % bad
    bad = [(i, len(d)) for i, d in enumerate(bufs) if whole[i] != want[i]]
    assert not bad, "ZS_NO_SPLIT_BACKEND differs from the oracle: %r" % bad
    return want


def _symbols(z):
    """symbols of every block of a stream of coded blocks, END_BLOCK not counted"""
    return [len(b.symbols) for b in deflate_reader.read(z)]


@pytest.fixture(scope="module")
def spec_exe():
    return model.build_model()


def _body_syms(spec_exe, path, data, level=6):
    """what the CPU model says the bulk parse emits (StreamState::body_syms): the tail engine's first symbol is the next one"""
    path.write_bytes(data)
    r = subprocess.run([spec_exe, str(path), str(level), "0", "1024", "128"], capture_output=True, text=True)
    m = re.search(r"^PASS .*path=spec .* syms=(\d+)", r.stdout, re.M)
    assert r.returncode == 0 and m, r.stdout[-400:]
    return int(m.group(1))


def test_no_finished_block(engine, oracle):
    """66 000 bytes of text from a vocabulary of 150 words: the stream walks and verifies (the CPU model says so), its parse has
    12 187 symbols, nb_body = 0 and part 0 is empty"""
    rng = np.random.default_rng(3)
    words = model.alice_of(152089).split()
    vocab = [words[i] + b" " for i in rng.integers(0, len(words), 150)]
    data = b"".join(vocab[i] for i in rng.integers(0, 150, 30000))[:66000]
    (want,) = _check(engine, oracle, [data], ZS_SPEC_MIN=65536)
    assert (engine.counter("spec_streams"), engine.counter("spec_fallbacks")) == (1, 0)
    assert sum(_symbols(want)) < BLOCK


# alice29.txt repeated and cut: around 99 400 bytes the second block cut (symbol 32766) passes the hand-over
CUT_LENGTHS = (99129, 99381, 99384, 99390, 99391, 99399, 99400, 99406)


def test_the_last_cut_around_the_hand_over(engine, oracle, spec_exe, tmp_path):
    """The last block cut against the tail engine's first symbol (symbol number body_syms, counted from 0): the cut falls (a) at
    least one symbol in front of it, (b) exactly on the last body symbol -- body_syms a multiple of 16383, the tail engine opens
    a fresh block --, (c) on the tail engine's first symbol, (d) inside the tail.  body_syms is the CPU model's, the symbols per
    block are read from the oracle's stream; every class must be present among the lengths."""
    classes = {}
    datas = [model.alice_of(n) for n in CUT_LENGTHS]
    wants = _check(engine, oracle, datas[:1], ZS_SPEC_MIN=65536)
    for d in datas[1:]:
        wants += _check(engine, oracle, [d], ZS_SPEC_MIN=65536)
    for n, d, z in zip(CUT_LENGTHS, datas, wants):
        total, body = sum(_symbols(z)), _body_syms(spec_exe, tmp_path / "m", d)
        cut = BLOCK * (total // BLOCK)  # symbols in front of the last cut: its last one is symbol cut - 1
        assert cut >= BLOCK and body <= total
        cls = "a" if cut < body else "b" if cut == body else "c" if cut == body + 1 else "d"
        classes.setdefault(cls, []).append((n, total, body))
    print(classes)
    assert sorted(classes) == ["a", "b", "c", "d"], classes
    # (and the stream whose last symbol completes a block: the eof block is empty)
    assert any(total % BLOCK == 0 for v in classes.values() for _, total, _ in v), classes


def test_stored_blocks_in_the_body(engine, oracle):
    """200 KiB of random bytes at level 6: stored blocks, thread 0's walk in both parts of K8 and Copy_block in both parts of K9"""
    data = np.random.default_rng(5).integers(0, 256, 200 << 10, dtype=np.uint8).tobytes()
    (want,) = _check(engine, oracle, [data], ZS_SPEC_MIN=65536)
    kinds = [b.kind for b in deflate_reader.read(want)]
    assert kinds.count("stored") >= 3, kinds


def test_a_mixed_call(oracle):
    """Three streams in one call: one that walks and verifies, one whose verification is spoiled and so takes the maps (chunk 150
    exists in it alone), one of 10 KiB.  (With a stream on the maps K5 runs beside the tail engine and the call keeps its one
    launch per kernel: test_a_stream_that_does_not_split_in_a_call_that_does has the two kinds of stream in a call that splits.)"""
    engine = Engine(0)
    try:
        a, b = model.alice_of(120000), model.alice_of(200000)[7:]
        bufs = [a, b, a[:10 << 10]]
        _check(engine, oracle, bufs, ZS_SPEC_MIN=65536, ZS_SPEC_CORRUPT=150)
        assert (engine.counter("spec_streams"), engine.counter("spec_fallbacks")) == (2, 1)
    finally:
        engine.close()


@pytest.mark.parametrize("strategy", [0, 1])
@pytest.mark.parametrize("level", [4, 6, 9])
def test_levels_and_strategies(engine, oracle, level, strategy):
    _check(engine, oracle, [model.alice_of(150001)], level, strategy, ZS_SPEC_MIN=65536)
    _check(engine, oracle, [model.alice_of(150001)], level, strategy)  # (below the default minimum: the maps)


def test_a_write_list_or_a_flush_mode_does_not_split(engine, oracle):
    data = model.alice_of(100 << 10)
    half = len(data) // 2

    def writes():
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        out = torch.zeros(deflate_bound(len(data)), dtype=torch.uint8, device="cuda")
        n = engine.deflate_writes_device(t.data_ptr(), len(data), [half, len(data)], out.data_ptr(), out.numel(), level=6)
        return out[:n].cpu().numpy().tobytes()

    def flushed():
        sink = io.BytesIO()
        s = ZlibOutputStream(sink, ZlibOptions(CompressionLevel=CompressionLevel(6), CompressionStrategy=CompressionStrategy(0), FlushMode=2), engine=engine)
        s.write(data[:half])
        s.Options.FlushMode = 0
        s.write(data[half:])
        s.close()
        return sink.getvalue()

    for z in _both(writes):
        assert z == oracle.compress(data, 6, 0, chunks=[half, len(data) - half])
    for z in _both(flushed):
        assert z == oracle.compress_writes(data, 6, 0, [half, len(data) - half], [2, 0])


def test_a_stream_that_does_not_split_in_a_call_that_does(oracle):
    """Level 3, where no kernel runs beside the tail engine: a plain stream, which splits, and one written in two Writes, which is
    part 1 entirely and reads the symbols the main stream placed.  The call times its part-1 chain: it split."""
    engine = Engine(0)
    try:
        engine.set_profiling(True)
        a, b = model.alice_of(140000), model.alice_of(150000)[5000:]
        tin = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in (a, b)]
        caps = [deflate_bound(len(a)), deflate_bound(len(b))]
        want = [oracle.compress(a, 3), oracle.compress(b, 3, 0, chunks=[70000, len(b) - 70000])]

        def call():
            outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
            lens = engine.deflate_writes_batch_device([t.data_ptr() for t in tin], [len(a), len(b)], [None, [70000, len(b)]], [o.data_ptr() for o in outs], caps, level=3)
            return [o[:n].cpu().numpy().tobytes() for o, n in zip(outs, lens)], engine.stage_ms()["part1_chain"]

        (z, chain), (z0, chain0) = _both(call)
        assert z == want and z0 == want
        assert chain > 0 and chain0 == 0
    finally:
        engine.close()


def test_capacity(oracle):
    """out_cap one byte short, half, and 8: ZS_BUF_ERROR, nothing written from out + out_cap on; the same call with room is the
    oracle's, so part 0 of a refused call leaves nothing behind"""
    engine = Engine(0)
    try:
        data = model.alice_of(180000)
        want = oracle.compress(data, 6)
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        room = deflate_bound(len(data))

        def call(cap):
            out = torch.full((room,), 0xA5, dtype=torch.uint8, device="cuda")
            rc, lens, status = engine.deflate_writes_batch_device([t.data_ptr()], [len(data)], None, [out.data_ptr()], [cap], level=6, return_status=True)
            torch.cuda.synchronize()
            return rc, lens[0], status[0], out.cpu().numpy()

        for no_split in (False, True):
            env = {"ZS_NO_SPLIT_BACKEND": 1} if no_split else {}
            for cap in (len(want) - 1, len(want) // 2, 8):
                rc, n, status, out = _with_env(lambda: call(cap), ZS_SPEC_MIN=65536, **env)
                assert rc != 0 and status == ZS_BUF_ERROR, (no_split, cap, rc, status)
                assert (out[cap:] == 0xA5).all(), (no_split, cap, int(np.flatnonzero(out[cap:] != 0xA5)[0]) + cap)
                rc, n, status, out = _with_env(lambda: call(room), ZS_SPEC_MIN=65536, **env)
                assert rc == 0 and status == 0 and out[:n].tobytes() == want, (no_split, cap)
            # (exactly enough: the finished blocks next to the end are part 1's)
            rc, n, status, out = _with_env(lambda: call(len(want)), ZS_SPEC_MIN=65536, **env)
            assert rc == 0 and status == 0 and out[:n].tobytes() == want and (out[len(want):] == 0xA5).all(), no_split
    finally:
        engine.close()


def test_the_call_splits_and_the_switch_keeps_it_whole(oracle):
    """stage_ms: a call that splits times its part-1 chain on the second stream; with a stream on the maps, under
    ZS_NO_SPLIT_BACKEND, for a batch of 64 streams (the live block list) and for a stream too short for a finished block there
    is no such chain"""
    engine = Engine(0)
    try:
        engine.set_profiling(True)
        data = model.alice_of(150000)

        def chain(bufs, **env):
            z = _with_env(lambda: engine.deflate_batch(bufs, level=6), **env)
            assert z == [oracle.compress(d, 6) for d in bufs]
            return engine.stage_ms()["part1_chain"]

        walk = {"ZS_SPEC_MIN": 65536}
        assert chain([data], **walk) > 0
        assert chain([data]) == 0  # (below the walk's default minimum: the maps, K5 beside the tail engine)
        assert chain([data], ZS_NO_SPLIT_BACKEND=1, **walk) == 0
        assert chain([data[:16000]], **walk) == 0
        many = [data[1000 * i:1000 * i + 66000] for i in range(64)]
        assert chain(many, **walk) == 0
        assert chain(many[:63], **walk) > 0
    finally:
        engine.close()


def test_the_same_shape_twice(oracle):
    """the kept plan gives the second call's bytes"""
    engine = Engine(0)
    try:
        a, b = model.alice_of(131072), model.alice_of(131072 + 4099)[4099:]
        for no_split in (False, True):
            env = {"ZS_NO_SPLIT_BACKEND": 1} if no_split else {}
            za = _with_env(lambda: engine.deflate_batch([a], level=6), ZS_SPEC_MIN=65536, **env)[0]
            zb = _with_env(lambda: engine.deflate_batch([b], level=6), ZS_SPEC_MIN=65536, **env)[0]
            assert engine.counter("plan_reused") == 1
            assert za == oracle.compress(a, 6) and zb == oracle.compress(b, 6), no_split
    finally:
        engine.close()
