"""The speculative chunk walk of levels 4-9 against the oracle and against the transfer maps forced by
ZS_NO_SPEC: the bytes never depend on the path, the counters say which path ran, and what the walk leaves for the kernels
behind it is what the maps leave."""
import ctypes
import hashlib
import io
import os

import numpy as np
import pytest

import oracle_binding
import test_spec_model as model
from zlibstream_amd import Engine, ZlibOptions, ZlibOutputStream, _native, datagen, deflate_bound

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


def _deflate(engine, bufs, level=6, strategy=0, hash_variant=0, **env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        z = engine.deflate_batch(bufs, level=level, strategy=strategy, hash_variant=hash_variant)
    finally:
        for k in env:
            os.environ.pop(k, None)
    return z, {k: engine.counter(k) for k in ("spec_streams", "spec_fallbacks", "spec_wrong_chunks")}


_ORACLE = {}


def _ref(oracle, data, level=6, strategy=0, hash_variant=0):
    """the oracle's stream, made once per (data, level, strategy, hash_variant): it does ~26 MB/s and the spoiled-guess cases ask
    for the same buffer many times"""
    key = (len(data), hashlib.sha1(data).digest(), level, strategy, hash_variant)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.compress(data, level, strategy, hash_variant=hash_variant)
    return _ORACLE[key]


VERIFIED = {"spec_streams": 1, "spec_fallbacks": 0, "spec_wrong_chunks": 0}
ONE_WRONG = {"spec_streams": 1, "spec_fallbacks": 1, "spec_wrong_chunks": 1}


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


# ---------------------------------------------------------------------------------------------------------------------------
# The walk at its edges.  A single Write of n bytes, chunks of L: body_end = n - 262; the grid has ((n - 1) >> log2 L) + 1 chunks;
# chunk j >= 1 is [j L - 261, (j + 1) L - 261) cut at n - 261; window end k fires at 65536 + 32768 k - 261, the first position
# of chunk (65536 + 32768 k) / L.  The verdict kernel takes 8192 chunks a tile, 8 a thread, 512 a wave; the walk 64 a workgroup.

@pytest.fixture(scope="module")
def spec_exe():
    return model.build_model()


def _left(engine):
    """what the parse leaves for the kernels behind it: the tail engine's state and the block cuts"""
    return {"state": _debug(engine, "state", np.int32, 6).tolist(), "blk_end": _debug(engine, "blk_end", np.int32, 4096).tolist(),
            "blk_top": _debug(engine, "blk_top", np.int32, 4096).tolist()}


def _walk_against_maps(engine, oracle, data, level, length, fallbacks, **env):
    """One stream down the walk and down the maps: the bytes, the oracle's, and what either leaves.  Returns what is wrong."""
    (z,), cnt = _deflate(engine, [data], level, ZS_SPEC_LEN=length, **env)
    left = _left(engine)
    (z0,), cnt0 = _deflate(engine, [data], level, ZS_NO_SPEC=1)
    left0 = _left(engine)
    bad = []
    if z != _ref(oracle, data, level):
        bad.append("bytes differ from the oracle's")
    if z0 != z:
        bad.append("bytes differ from the maps'")
    if cnt0["spec_streams"] != 0:
        bad.append("ZS_NO_SPEC walked")
    if (cnt["spec_streams"], cnt["spec_fallbacks"]) != (1, fallbacks):
        bad.append("counters %r (periodic %d), expected %d fallback(s)" % (cnt, _periodic(engine), fallbacks))
    for k in left:
        if left[k] != left0[k]:
            bad.append("%s differs from what the maps leave" % k)
    return bad


@pytest.mark.parametrize("length", [512, 1024, 2048])
@pytest.mark.parametrize("level", [6, 9])
def test_lengths_on_the_speculative_grid(engine, oracle, level, length):
    """The 63 lengths of tests/test_spec_model.py grid_lengths() -- a window end within 263 bytes either side of the stream's
    end, a last chunk of zero, one and two positions -- with the shortest walked stream lowered to 64 KiB.  The CPU model says
    every one of them verifies (test_spec_model.py test_lengths_on_the_speculative_grid), so a fallback here is a finding."""
    lens = model.grid_lengths()
    assert len(lens) == 63
    bad = {}
    for n in lens:
        b = _walk_against_maps(engine, oracle, model.alice_of(n), level, length, 0, ZS_SPEC_MIN=65536)
        if b:
            bad[n] = b
    assert not bad, bad


@pytest.mark.parametrize("length", [1024, 512])
def test_lengths_on_the_speculative_grid_above_1_mib(engine, oracle, spec_exe, tmp_path, length):
    """The same two families from 1 MiB on, where the walk is on by itself (level 6; no ZS_SPEC_MIN): window ends 31..33 and
    j L + 0, 1, 2 from exactly 1 MiB.  The verdict is the model's, asked at test time."""
    lens = model.grid_lengths(big=True)
    assert len(lens) == 45 and lens[0] == 1 << 20
    jobs = []
    for n in lens:
        (tmp_path / str(n)).write_bytes(model.alice_of(n))
        jobs.append((spec_exe, str(tmp_path / str(n)), 6, 0, str(length)))
    verdicts = [r[length] for r in model._all(jobs, model.run_model)]
    assert sum(v["path"] == "spec" for v in verdicts) >= 40, verdicts  # (all 45, when this was written)
    bad = {}
    for n, v in zip(lens, verdicts):
        b = _walk_against_maps(engine, oracle, model.alice_of(n), 6, length, 0 if v["path"] == "spec" else 1)
        if v["path"] != "spec" and not v["bail"] and engine.counter("spec_wrong_chunks") != v["wrong"]:
            b.append("model: %d wrong guesses" % v["wrong"])
        if b:
            bad[n] = b
    assert not bad, bad


@pytest.fixture(scope="module")
def english12():
    return datagen.english(12 << 20)


def _spoil(engine, oracle, data, level, strategy, length, chunks):
    """ZS_SPEC_CORRUPT changes the recorded guess of one chunk, not the walk: exactly one comparison of the verdict fails, the
    stream goes to the maps and is the oracle's all the same."""
    n = ((len(data) - 1) // length) + 1
    (z,), cnt = _deflate(engine, [data], level, strategy, ZS_SPEC_LEN=length)
    assert cnt == VERIFIED and z == _ref(oracle, data, level, strategy), cnt
    bad = {}
    for j in chunks:
        assert 0 <= j < n
        (z,), cnt = _deflate(engine, [data], level, strategy, ZS_SPEC_LEN=length, ZS_SPEC_CORRUPT=j)
        if cnt != ONE_WRONG or z != _ref(oracle, data, level, strategy):
            bad[j] = (cnt, "the oracle's bytes" if z == _ref(oracle, data, level, strategy) else "NOT the oracle's bytes")
    assert not bad, bad
    # beyond the grid: nothing is spoiled
    (z,), cnt = _deflate(engine, [data], level, strategy, ZS_SPEC_LEN=length, ZS_SPEC_CORRUPT=n)
    assert cnt == VERIFIED and z == _ref(oracle, data, level, strategy), cnt


def test_a_spoiled_guess_on_every_seam(engine, oracle, english12):
    """9 MiB + 1 byte in chunks of 512: 18 433 chunks, three tiles of the verdict kernel, the last chunk one position long (and the
    first of window end 286).  The spoiled chunk is the first (its entry is checked against the initial state), either side of a
    thread's 8, a workgroup's 64, a wave's 512, a tile's 8192, a window end's first chunk, and the last two."""
    data = english12[:(9 << 20) + 1]
    n = 18433
    ends = [(65536 + 32768 * k) // 512 for k in (1, 150)]
    assert ends == [192, 9728]
    chunks = [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 16383, 16384] + [e + d for e in ends for d in (-1, 0, 1)] + [n - 2, n - 1]
    _spoil(engine, oracle, data, 6, 0, 512, chunks)


@pytest.mark.parametrize("length,chunks", [(1024, [0, 1, 8, 64, 96, 511, 512, 8191, 8192, 8193, 9215, 9216]),
                                           (2048, [0, 7, 8, 48, 63, 64, 512, 4607, 4608])])
def test_a_spoiled_guess_on_the_seams_of_longer_chunks(engine, oracle, english12, length, chunks):
    data = english12[:(9 << 20) + 1]
    assert chunks[-1] == (len(data) - 1) // length  # the last chunk, one position long
    _spoil(engine, oracle, data, 6, 0, length, chunks)


@pytest.mark.parametrize("level,strategy", [(9, 0), (6, 1)])
def test_a_spoiled_guess_at_level_9_and_filtered(engine, oracle, english12, level, strategy):
    _spoil(engine, oracle, english12[:(9 << 20) + 1], level, strategy, 512, [8192, 9728, 18432])


def test_a_spoiled_guess_in_every_stream_of_a_batch(engine, oracle, english12):
    """The switch spoils chunk j of every stream that has one.  3 MiB, 9 MiB and 1 MiB + 1 byte in chunks of 1024 (3072, 9216 and
    1025 chunks; the streams behind the first read their records at spec_off != 0).  j = 2000: the third stream verifies, and its
    symbols survive its neighbours' way through the maps.  j = 1024: the third stream's last chunk, one position long."""
    bufs = [english12[:3 << 20], english12[(3 << 20):(12 << 20)], english12[(5 << 20):(6 << 20) + 1]]
    want = [_ref(oracle, d) for d in bufs]
    z, cnt = _deflate(engine, bufs, 6, ZS_SPEC_LEN=1024)
    assert cnt == {"spec_streams": 3, "spec_fallbacks": 0, "spec_wrong_chunks": 0} and z == want, cnt
    z, cnt = _deflate(engine, bufs, 6, ZS_SPEC_LEN=1024, ZS_SPEC_CORRUPT=2000)
    assert cnt == {"spec_streams": 3, "spec_fallbacks": 2, "spec_wrong_chunks": 2}, cnt
    assert z == want
    z, cnt = _deflate(engine, bufs, 6, ZS_SPEC_LEN=1024, ZS_SPEC_CORRUPT=1024)
    assert cnt == {"spec_streams": 3, "spec_fallbacks": 3, "spec_wrong_chunks": 3}, cnt
    assert z == want
    z, cnt = _deflate(engine, bufs, 6, ZS_SPEC_LEN=1024, ZS_SPEC_CORRUPT=0)
    assert cnt == {"spec_streams": 3, "spec_fallbacks": 3, "spec_wrong_chunks": 3}, cnt
    assert z == want


@pytest.mark.parametrize("warm", [0, 8, 32])
def test_naturally_wrong_guesses_are_the_models(engine, oracle, spec_exe, warm):
    """lcet10.txt with warm-ups too short to fall into step: the guesses are wrong by the data, not by a switch.  The stream is
    the oracle's by way of the maps, and the device counts the wrong guesses the CPU model counts (chunk
    j's guess is wrong when it is not chunk j - 1's exit, every chunk walked from its own guess)."""
    path = os.path.join(oracle_binding.CORPUS, "lcet10.txt")
    data = oracle_binding.corpus("lcet10.txt")
    assert len(data) == 419235
    want = model.run_model(spec_exe, path, 6, 0, model.LENS, warm)
    for length in (512, 1024, 2048):
        m = want[length]
        assert m["path"] == "maps" and m["wrong"] > 0, (length, m)
        (z,), cnt = _deflate(engine, [data], 6, ZS_SPEC_MIN=65536, ZS_SPEC_LEN=length, ZS_SPEC_WARM=warm)
        print("lcet10 warm %d chunks of %d: device %r, model %r" % (warm, length, cnt, m))
        assert z == _ref(oracle, data), (length, cnt)
        assert cnt["spec_streams"] == 1 and cnt["spec_fallbacks"] == 1 and _periodic(engine) == 0, (length, cnt)
        if not m["bail"]:
            assert cnt["spec_wrong_chunks"] == m["wrong"], (length, cnt, m)


# ---- what the suite never sent down this path ----

@pytest.mark.parametrize("size,level,strategy", [(2 << 20, 6, 0), (2 << 20, 9, 0), (8 << 20, 6, 0), (8 << 20, 9, 0), (8 << 20, 6, 1)])
def test_the_multiplicative_hash_takes_the_walk(engine, oracle, english8, size, level, strategy):
    """hash_variant=1 changes the chains, not the walk: the text verifies as it does under the reference's hash."""
    data = english8[:size]
    (z,), cnt = _deflate(engine, [data], level, strategy, hash_variant=1)
    assert z == _ref(oracle, data, level, strategy, 1), cnt
    assert z != _ref(oracle, data, level, strategy, 0)
    assert cnt == VERIFIED, cnt
    (z0,), cnt0 = _deflate(engine, [data], level, strategy, hash_variant=1, ZS_NO_SPEC=1)
    assert cnt0["spec_streams"] == 0 and z0 == z


@pytest.mark.parametrize("level", [5, 7])
def test_levels_5_and_7(engine, oracle, spec_exe, english8, tmp_path, level):
    data = english8[:3 << 20]
    (tmp_path / "english3").write_bytes(data)
    m = model.run_model(spec_exe, str(tmp_path / "english3"), level, 0, "1024")[1024]
    (z,), cnt = _deflate(engine, [data], level)
    assert z == _ref(oracle, data, level), cnt
    assert cnt["spec_streams"] == 1 and cnt["spec_fallbacks"] == (0 if m["path"] == "spec" else 1), (cnt, m)
    (z0,), cnt0 = _deflate(engine, [data], level, ZS_NO_SPEC=1)
    assert cnt0["spec_streams"] == 0 and z0 == z


def _text_with_rows(english8, tiles):
    """2 MiB (128 match tiles of 16 KiB): english with `tiles` tiles of image rows (512 pixels, 2048 bytes a row) from 1 MiB on"""
    rows = datagen.sparse(512, tiles * 8)
    data = english8[:1 << 20] + rows + english8[1 << 20:(2 << 20) - len(rows)]
    assert len(data) == 2 << 20 and len(rows) == tiles * 16384
    return data


@pytest.mark.parametrize("tiles,periodic", [(6, 0), (43, 1), (15, None), (17, None)])
def test_text_with_image_rows_inside(engine, oracle, english8, tiles, periodic):
    """A stream is not walked when more than 1 / 8 of its match tiles are on the match kernel's RUNS walk.  About 1 / 20 of the
    tiles in rows: walked (verified or bailed, the bytes decide); about 1 / 3: periodic.  Which tiles the match kernel counts
    is its business, so near 1 / 8 (15 and 17 of 128) only the bytes are asserted."""
    data = _text_with_rows(english8, tiles)
    (z,), cnt = _deflate(engine, [data], 6)
    per = _periodic(engine)
    print("%d of 128 tiles in rows: %r, periodic %d" % (tiles, cnt, per))
    assert z == _ref(oracle, data), cnt
    assert cnt["spec_streams"] == 1
    if periodic is not None:
        assert per == periodic, cnt
        assert cnt["spec_fallbacks"] >= periodic and (periodic == 0 or cnt["spec_wrong_chunks"] == 0), cnt
    (z0,), cnt0 = _deflate(engine, [data], 6, ZS_NO_SPEC=1)
    assert cnt0["spec_streams"] == 0 and z0 == z


@pytest.mark.parametrize("shorts,walked", [(8, 1), (200, 0), (35, None), (36, None)])
def test_one_long_stream_among_short_ones(engine, oracle, english8, shorts, walked):
    """The walk's grids are (chunks of the longest stream / 64) x streams, so a batch of one long stream and many short ones
    keeps the maps: 8 MiB is 128 workgroups, and the walk is off when 128 n > 4 * 128 + 4096 -- on for 9 streams, off for 201.
    Either side of the rule's edge (36 and 37 streams) the bytes only: the constant may be retuned."""
    bufs = [english8[5000 * i:5000 * i + 3000 + 7 * i] for i in range(shorts)]
    bufs.insert(shorts // 2, english8)
    z, cnt = _deflate(engine, bufs, 6)
    assert z == [_ref(oracle, d) for d in bufs], cnt
    if walked is not None:
        assert cnt == {"spec_streams": walked, "spec_fallbacks": 0, "spec_wrong_chunks": 0}, cnt
    z0, cnt0 = _deflate(engine, bufs, 6, ZS_NO_SPEC=1)
    assert cnt0["spec_streams"] == 0 and z0 == z


@pytest.mark.parametrize("front", [1, 15, 17, 4097])
def test_walked_streams_behind_odd_lengths(engine, oracle, english12, front):
    """The stream's offset into the batch's records decides how the lane's ring is aligned (pos_off & 15)."""
    bufs = [english12[:front], english12[(1 << 20):(2 << 20) + 3], english12[7:front + 7], english12[(2 << 20):(4 << 20) - 1]]
    z, cnt = _deflate(engine, bufs, 6)
    assert cnt == {"spec_streams": 2, "spec_fallbacks": 0, "spec_wrong_chunks": 0}, cnt
    assert z == [_ref(oracle, d) for d in bufs]
    z0, _ = _deflate(engine, bufs, 6, ZS_NO_SPEC=1)
    assert z0 == z


@pytest.mark.parametrize("order", [0, 1])
def test_walked_streams_of_very_different_lengths(engine, oracle, english12, order):
    """1 MiB beside 12 MiB: most lanes of the shorter stream's grid return at once, the longer has two tiles of the verdict."""
    bufs = [english12[(3 << 20):(4 << 20)], english12]
    bufs = bufs[::-1] if order else bufs
    z, cnt = _deflate(engine, bufs, 6, ZS_SPEC_LEN=1024)
    assert cnt == {"spec_streams": 2, "spec_fallbacks": 0, "spec_wrong_chunks": 0}, cnt
    assert z == [_ref(oracle, d) for d in bufs]
    z0, _ = _deflate(engine, bufs, 6, ZS_NO_SPEC=1)
    assert z0 == z


def test_ragged_streams_at_odd_device_pointers(engine, oracle, english12):
    """deflate_batch_device: three walked streams that are slices of one tensor at offsets 1, 3 and 7."""
    import torch
    lens = [(1 << 20) + 1, (2 << 20) + 333, (3 << 20) - 5]
    offs = [1, 3, 7]
    host = english12[:offs[-1] + lens[-1]]
    d_in = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
    outs = [torch.empty(deflate_bound(n), dtype=torch.uint8, device="cuda") for n in lens]
    assert all((d_in.data_ptr() + o) & 1 for o in offs)
    got = engine.deflate_batch_device([d_in.data_ptr() + o for o in offs], lens, [t.data_ptr() for t in outs], [t.numel() for t in outs],
                                      level=6, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cnt = {k: engine.counter(k) for k in ("spec_streams", "spec_fallbacks", "spec_wrong_chunks")}
    assert cnt == {"spec_streams": 3, "spec_fallbacks": 0, "spec_wrong_chunks": 0}, cnt
    for o, n, t, m in zip(offs, lens, outs, got):
        assert t[:m].cpu().numpy().tobytes() == _ref(oracle, host[o:o + n])
