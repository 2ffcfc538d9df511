"""The speculative chunk walk of levels 4-9 against the oracle and against the transfer maps forced by
ZS_NO_SPEC: the bytes never depend on the path, the counters say which path ran, and what the walk leaves for the kernels
behind it is what the maps leave."""
import ctypes
import io
import os

import numpy as np
import pytest

import oracle_binding
from zlibstream_amd import Engine, ZlibOptions, ZlibOutputStream, _native, datagen

pytestmark = pytest.mark.gpu

SWITCHES = ("ZS_NO_SPEC", "ZS_SPEC_CORRUPT", "ZS_SPEC_LEN", "ZS_SPEC_WARM", "ZS_SPEC_MIN", "ZS_FORCE_ROUNDS")


@pytest.fixture(autouse=True)
def _clean_env():
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _deflate(engine, bufs, level=6, strategy=0, **env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        z = engine.deflate_batch(bufs, level=level, strategy=strategy)
    finally:
        for k in env:
            os.environ.pop(k, None)
    return z, {k: engine.counter(k) for k in ("spec_streams", "spec_fallbacks", "spec_wrong_chunks")}


def _periodic(engine):
    """streams of the last call that were never walked: the match kernel's count of tiles on the RUNS walk said so"""
    return engine.counter("spec_periodic")


def _repeat(name, to=2 << 20):
    d = oracle_binding.corpus(name)
    return d * (to // len(d) + 1)


@pytest.fixture(scope="module")
def english8():
    return datagen.english(8 << 20)


@pytest.mark.parametrize("level", [4, 6, 8, 9])
@pytest.mark.parametrize("strategy", [0, 1])
def test_text_takes_the_speculative_walk_bit_exact(engine, oracle, english8, level, strategy):
    for data in (english8[:1 << 20], english8):
        (z,), cnt = _deflate(engine, [data], level, strategy)
        assert cnt == {"spec_streams": 1, "spec_fallbacks": 0, "spec_wrong_chunks": 0}, cnt
        assert z == oracle.compress(data, level, strategy)
        (z0,), cnt0 = _deflate(engine, [data], level, strategy, ZS_NO_SPEC=1)
        assert cnt0["spec_streams"] == 0 and z0 == z


@pytest.fixture(scope="module")
def english64():
    return datagen.english(64 << 20)


@pytest.mark.parametrize("level", [4, 6, 8, 9])
@pytest.mark.parametrize("strategy", [0, 1])
def test_english64_takes_the_speculative_walk_bit_exact(engine, oracle, english64, level, strategy):
    """The headline buffer, whole: equal to the oracle and to the maps, no fallback, no wrong guess."""
    (z,), cnt = _deflate(engine, [english64], level, strategy)
    assert cnt == {"spec_streams": 1, "spec_fallbacks": 0, "spec_wrong_chunks": 0}, cnt
    (z0,), cnt0 = _deflate(engine, [english64], level, strategy, ZS_NO_SPEC=1)
    assert cnt0["spec_streams"] == 0 and z == z0
    assert z == oracle.compress(english64, level, strategy)


@pytest.mark.parametrize("name", sorted(os.listdir(oracle_binding.CORPUS)))
def test_corpus_files_repeated_to_2_mib(engine, oracle, name):
    data = _repeat(name)
    (z,), cnt = _deflate(engine, [data], 6)
    assert z == oracle.compress(data, 6), cnt
    (z0,), _ = _deflate(engine, [data], 6, ZS_NO_SPEC=1)
    assert z0 == z


@pytest.mark.parametrize("length,warm", [(512, 128), (512, 256), (1024, 64), (1024, 256), (2048, 128), (2048, 256)])
def test_every_chunk_length_and_warmup(engine, oracle, english8, length, warm):
    data = english8[:3 << 20]
    (z,), cnt = _deflate(engine, [data], 6, ZS_SPEC_LEN=length, ZS_SPEC_WARM=warm)
    assert cnt["spec_streams"] == 1 and cnt["spec_fallbacks"] == 0, cnt
    assert z == oracle.compress(data, 6)


def test_periodic_data_stays_with_the_maps_and_no_lane_walks(engine, oracle):
    """Image rows: the match kernel's count of tiles on the RUNS walk keeps the stream off the path -- it is counted as a stream
    that fell back, and the verdict says "periodic": no lane of it walked."""
    for data in (datagen.sparse(2048, 2048), datagen.batch_buffer(1, 1 << 20)):
        (z,), cnt = _deflate(engine, [data], 6)
        assert cnt == {"spec_streams": 1, "spec_fallbacks": 1, "spec_wrong_chunks": 0}, cnt
        assert _periodic(engine) == 1
        (z0,), _ = _deflate(engine, [data], 6, ZS_NO_SPEC=1)
        assert z == z0
        assert z == oracle.compress(data, 6)


def test_zeros_in_the_middle_of_text_bail_to_the_maps(engine, oracle, english8):
    """64 KiB of zeros between two MiB of text: read events whose loop-top shares its bucket with the next position cut chains,
    which is the resolve kernel's business."""
    data = english8[:1 << 20] + bytes(65536) + english8[1 << 20:2 << 20]
    (z,), cnt = _deflate(engine, [data], 6)
    assert cnt["spec_streams"] == 1 and cnt["spec_fallbacks"] == 1, cnt
    assert z == oracle.compress(data, 6)


@pytest.mark.parametrize("level", [6, 9])
def test_a_verified_stream_beside_one_in_the_cut_rounds(engine, oracle, english8, level):
    """A text stream that verifies in one batch with zero pages that the resolve kernel gives up to the batched cut rounds: the
    call re-enters behind the rounds without launching anything of the speculative path again, and the verified stream's
    symbols and block cuts are those of the first pass."""
    bufs = [english8[:2 << 20], bytes(4 << 20), english8[(2 << 20):(3 << 20) + 777]]
    before = engine.counter("round_runs")
    z, cnt = _deflate(engine, bufs, level, ZS_FORCE_ROUNDS=1)
    assert engine.counter("round_runs") > before
    assert cnt["spec_streams"] == 3 and cnt["spec_fallbacks"] == 1, cnt
    for d, got in zip(bufs, z):
        assert got == oracle.compress(d, level)
    z0, _ = _deflate(engine, bufs, level, ZS_NO_SPEC=1, ZS_FORCE_ROUNDS=1)
    assert z0 == z


def test_a_spoiled_guess_sends_the_stream_to_the_maps(engine, oracle, english8):
    (z,), cnt = _deflate(engine, [english8], 6, ZS_SPEC_CORRUPT=777)
    assert cnt == {"spec_streams": 1, "spec_fallbacks": 1, "spec_wrong_chunks": 1}, cnt
    assert z == oracle.compress(english8, 6)


def test_a_batch_that_mixes_all_of_them(engine, oracle, english8):
    zeros_mid = english8[:1 << 20] + bytes(65536) + english8[1 << 20:2 << 20]
    bufs = [english8[:1 << 20], datagen.batch_buffer(1, 1 << 20), _repeat("ptt5"), english8[:3 << 20], zeros_mid, english8[:500000], b"",
            _repeat("kennedy.xls"), english8[:(1 << 20) + 12345]]
    z, cnt = _deflate(engine, bufs, 6)
    assert cnt["spec_streams"] >= 5 and 0 < cnt["spec_fallbacks"] < cnt["spec_streams"], cnt
    for d, got in zip(bufs, z):
        assert got == oracle.compress(d, 6)
    z0, _ = _deflate(engine, bufs, 6, ZS_NO_SPEC=1)
    assert z0 == z


@pytest.mark.parametrize("flush", [0, 2])
def test_streams_that_do_not_qualify(engine, oracle, english8, flush):
    """Several Writes, Writes under a flush mode (every run behind a flush is a resumed one): the maps, the same bytes."""
    data = english8[:4 << 20]
    sizes = [1536 << 10, 1 << 20, (4 << 20) - (1536 << 10) - (1 << 20)]
    engine.deflate_batch([b"abc"], level=6)  # (the counters are those of the last call: none of a test before)
    sink = io.BytesIO()
    zs = ZlibOutputStream(sink, ZlibOptions(CompressionLevel=6, FlushMode=flush), engine=engine)
    at = 0
    seen = 0
    for s in sizes:
        zs.write(data[at:at + s])
        seen += engine.counter("spec_streams")
        at += s
    zs.Finish()
    seen += engine.counter("spec_streams")
    zs.close()
    assert seen == 0
    assert sink.getvalue() == oracle.compress(data, 6, 0, chunks=sizes, flush=flush)


def _debug(engine, name, dtype, n):
    lib = _native.lib()
    buf = np.zeros(n, dtype=dtype)
    got = lib.zs_ctx_debug_read(engine.handle, name.encode(), buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes)
    assert got >= 0, name
    return buf[:got // buf.itemsize]


@pytest.mark.parametrize("length", [512, 1024, 2048])
def test_what_the_walk_leaves_is_what_the_maps_leave(engine, english8, length):
    """english 8 MiB: the stream's state for the tail engine (tail_p, tail_kind, tail_pend, k_done, preins, body_syms), the
    block cuts blk_end / blk_top and the chunks' first symbols, field by field."""
    nch = (8 << 20) // 512 + 8
    (z,), cnt = _deflate(engine, [english8], 6, ZS_SPEC_LEN=length)
    assert cnt["spec_streams"] == 1 and cnt["spec_fallbacks"] == 0
    state = _debug(engine, "state", np.int32, 6).copy()
    ends, tops = _debug(engine, "blk_end", np.int32, 4096).copy(), _debug(engine, "blk_top", np.int32, 4096).copy()
    base = _debug(engine, "spec_base", np.uint32, nch).copy()
    (z0,), _ = _deflate(engine, [english8], 6, ZS_NO_SPEC=1)
    state0 = _debug(engine, "state", np.int32, 6)
    ends0, tops0 = _debug(engine, "blk_end", np.int32, 4096), _debug(engine, "blk_top", np.int32, 4096)
    base0 = _debug(engine, "symbase", np.uint32, nch)
    assert z == z0
    assert state.tolist() == state0.tolist()
    assert len(ends) == state[5] // 16383 > 100
    assert ends.tolist() == ends0.tolist() and tops.tolist() == tops0.tolist()
    per = 2048 // length
    assert base[::per].tolist() == base0.tolist()
