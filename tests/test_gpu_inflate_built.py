"""Hand-built deflate streams (tests/deflate_builder.py) through the block-parallel inflate: streams no encoder emits -- every
code at its extremes, 15-bit codes, length 258 as 284 + 31, empty blocks in runs, deflate inside stored blocks, thousands of tiny
blocks, blocks beyond a million symbols, matches that copy matches, matches across the expand kernel's step edges, random
complete codes -- against the plaintext the builder kept (tests/test_deflate_builder.py: zlib and the oracle agree with it).

Bytes alone cannot tell who decoded a stream: what the block-parallel pass gives up on goes to the one-wave decoder, which is
right too.  zs_ctx_counter("inf_wave_streams") counts those streams, and every case states whether it is one."""
import io
import zlib

import pytest

import deflate_builder as db
from zlibstream_amd import ZlibInputStream, datagen

pytestmark = pytest.mark.gpu

MODES = {"default": None, "chain_walk": ("ZS_INF_CHAIN_WALK", "1"), "no_tokens": ("ZS_INF_MEASURE_DBG", "3")}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", db.case_names())
def test_built_stream_alone(engine, monkeypatch, name, mode):
    """One stream a call.  default: the bytes, and whether the block-parallel pass kept the stream.  chain_walk: the walking
    chain kernel for every stream.  no_tokens: every measured block through the lane decoder and zs_inf_cellflat_kernel, the
    path of blocks under 4 bits per symbol and of token buffers that find no room."""
    _, z, plain, fallback = db.case(name)
    if MODES[mode]:
        monkeypatch.setenv(*MODES[mode])  # (both are read per call)
    got = engine.inflate_batch([z], [len(plain)])
    wave, lane = engine.counter("inf_wave_streams"), engine.counter("inf_lane_streams")
    print("%s [%s]: %d -> %d bytes, inf_wave_streams %d, inf_lane_streams %d" % (name, mode, len(z), len(plain), wave, lane))
    assert len(got) == 1 and len(got[0]) == len(plain)
    assert got[0] == plain
    counted = len(z) >= db.PAR_MIN
    if mode == "default":
        assert wave == (1 if fallback and counted else 0)
    if mode == "no_tokens":  # (a lane decoder that refuses what it should take is right in every byte, too)
        assert wave == (1 if (fallback or name in db.NO_TOKENS_FALLBACK) and counted else 0)
    if mode == "no_tokens" and name in ("all_codes", "deep_codes", "dependent_chain"):
        assert lane >= 1


@pytest.mark.parametrize("order", ["catalogue", "reversed"])
def test_built_streams_in_one_batch(engine, order):
    """The kernels run over flat (stream, item) lists: every stream beside every kind of neighbour, and the count of the
    streams handed on is the sum of the cases' own."""
    cat = list(db.catalogue())
    if order == "reversed":
        cat.reverse()
    got = engine.inflate_batch([c[1] for c in cat], [len(c[2]) for c in cat])
    wave = engine.counter("inf_wave_streams")
    bad = [c[0] for c, g in zip(cat, got) if g != c[2]]
    assert not bad, bad
    assert wave == sum(1 for c in cat if c[3] and len(c[1]) >= db.PAR_MIN)


@pytest.mark.parametrize("name", [n for n in db.case_names() if n == "all_codes" or n.startswith(("empties_", "nested_"))])
def test_built_stream_through_zlib_input_stream(engine, name):
    """Read 70 000 bytes at a time.  With a BytesIO underneath the mirror feeds the whole stream, 8 KiB a call, before the
    first decode: a stream above 1 MiB has its end looked for on a prefix on the way (finder, measure and chain), and the
    call without input then decodes the whole stream at once -- nothing here is decoded piece by piece
    (tests/test_gpu_inflate_stream.py does that)."""
    _, z, plain, _ = db.case(name)
    s = ZlibInputStream(io.BytesIO(z), engine=engine)
    got = bytearray()
    while True:
        part = s.read(70000)
        if not part:
            break
        got += part
    assert bytes(got) == plain
    assert s.TotalIn == len(z) and s.TotalOut == len(plain) and s.Adler == zlib.adler32(plain)


def test_wave_counter_is_the_last_calls_and_counts_streams(engine):
    text = datagen.english(256 << 10, 5)
    z = zlib.compress(text, 6)
    _, dense, dense_plain, fallback = db.case("tiny_blocks_dense")
    assert fallback and len(z) >= db.PAR_MIN
    assert engine.inflate_batch([z, dense], [len(text), len(dense_plain)]) == [text, dense_plain]
    assert engine.counter("inf_wave_streams") == 1
    assert engine.inflate_batch([z], [len(text)]) == [text]
    assert engine.counter("inf_wave_streams") == 0  # an ordinary stream is the block-parallel pass's; the count is not a running sum
    assert engine.inflate_batch([dense] * 3 + [z], [len(dense_plain)] * 3 + [len(text)])[3] == text
    assert engine.counter("inf_wave_streams") == 3
    _, small, small_plain, _ = db.case("threshold_1023")
    assert engine.inflate_batch([small], [len(small_plain)]) == [small_plain]
    assert engine.counter("inf_wave_streams") == 0  # below the minimum: the one-wave decoder's, and not counted
