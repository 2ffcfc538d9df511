"""The speculative walk that keeps its symbols: the walk writes every chunk's symbols into a slab, and
behind the verdict zs_spec_compact_kernel moves them to their places and finds the block cuts.  Byte-exact against the oracle
and against the transfer maps forced by ZS_NO_SPEC; the expected verdict of a case is the CPU model's, asked at test time --
where the model says a stream verifies, a fallback is a failure."""
import ctypes
import os

import numpy as np
import pytest

import oracle_binding
import test_spec_model as model
from zlibstream_amd import Engine, _native, datagen

pytestmark = pytest.mark.gpu

SWITCHES = ("ZS_NO_SPEC", "ZS_SPEC_CORRUPT", "ZS_SPEC_LEN", "ZS_SPEC_WARM", "ZS_SPEC_MIN", "ZS_FORCE_ROUNDS")
BLOCK = 16383  # kBlockSyms


@pytest.fixture(autouse=True)
def _clean_env():
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _deflate(engine, bufs, level=6, **env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        z = engine.deflate_batch(bufs, level=level)
    finally:
        for k in env:
            os.environ.pop(k, None)
    return z, {k: engine.counter(k) for k in ("spec_streams", "spec_fallbacks", "spec_wrong_chunks")}


def _debug(engine, name, dtype, n):
    buf = np.zeros(n, dtype=dtype)
    got = _native.lib().zs_ctx_debug_read(engine.handle, name.encode(), buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes)
    assert got >= 0, name
    return buf[:got // buf.itemsize].copy()


def _left(engine):
    """what the parse leaves for the kernels behind it: the tail engine's state and the block cuts"""
    return {"state": _debug(engine, "state", np.int32, 6).tolist(), "blk_end": _debug(engine, "blk_end", np.int32, 4096).tolist(),
            "blk_top": _debug(engine, "blk_top", np.int32, 4096).tolist()}


@pytest.fixture(scope="module")
def spec_exe():
    return model.build_model()


def _verdicts(spec_exe, tmp_path, datas, level, length):
    """the CPU model's verdict for every buffer at one chunk length: True where the stream verifies"""
    jobs = []
    for i, d in enumerate(datas):
        (tmp_path / ("m%d" % i)).write_bytes(d)
        jobs.append((spec_exe, str(tmp_path / ("m%d" % i)), level, 0, str(length)))
    return [r[length]["path"] == "spec" for r in model._all(jobs, model.run_model)]


def _walk_against_maps(engine, oracle, data, level, verifies, **env):
    """One stream down the walk and down the maps: the bytes, the oracle's, and what either leaves.  Returns what is wrong and
    the walk's spec_base."""
    (z,), cnt = _deflate(engine, [data], level, **env)
    left = _left(engine)
    length = int(env.get("ZS_SPEC_LEN", 1024))
    base = _debug(engine, "spec_base", np.uint32, (len(data) - 1) // length + 1)
    (z0,), cnt0 = _deflate(engine, [data], level, ZS_NO_SPEC=1)
    left0 = _left(engine)
    bad = []
    if z != oracle.compress(data, level):
        bad.append("bytes differ from the oracle's")
    if z0 != z:
        bad.append("bytes differ from the maps'")
    if cnt0["spec_streams"] != 0:
        bad.append("ZS_NO_SPEC walked")
    if (cnt["spec_streams"], cnt["spec_fallbacks"]) != (1, 0 if verifies else 1):
        bad.append("counters %r, the model says the stream %s" % (cnt, "verifies" if verifies else "goes to the maps"))
    for k in left:
        if left[k] != left0[k]:
            bad.append("%s differs from what the maps leave" % k)
    return bad, base, left["state"][5]


def _one_match(k, more=0, seed=20240611):
    """96 KiB of seeded random bytes with bytes 300 .. 300 + k a copy of bytes 0 .. k: one match of length k, behind which the
    symbol index trails the position by k - 1 (but for the few three-byte matches random bytes hold).  `more`: that many
    matches of length 258 behind it, each another 257 positions of lag."""
    d = bytearray(np.random.default_rng(seed).integers(0, 256, 96 << 10, dtype=np.uint8).tobytes())
    d[300:300 + k] = d[0:k]
    for i in range(more):
        at = 1000 * (i + 1)
        d[at + 400:at + 658] = d[at:at + 258]
    return bytes(d)


def _sweep(engine, oracle, spec_exe, tmp_path, length, ks, more=0):
    datas = [_one_match(k, more) for k in ks]
    verdicts = _verdicts(spec_exe, tmp_path, datas, 6, length)
    assert sum(verdicts) >= len(ks) - 4, "the model sends the sweep to the maps: it proves nothing"
    bad, first, last, most = {}, 0, 0, 0
    for k, d, v in zip(ks, datas, verdicts):
        b, base, body_syms = _walk_against_maps(engine, oracle, d, 6, v, ZS_SPEC_MIN=65536, ZS_SPEC_LEN=length)
        if b:
            bad[k] = b
        if not v:
            continue
        starts = set(base.tolist())
        counts = np.diff(np.append(base, np.uint32(body_syms)))
        most = max(most, int(counts.max()))
        for blk in range(body_syms // BLOCK):
            g = BLOCK * (blk + 1) - 1  # the stream's symbol that completes block blk
            first += g in starts
            last += g + 1 in starts
    assert not bad, bad
    return first, last, most


def test_a_block_cut_at_every_alignment_to_a_chunk_boundary_512(engine, oracle, spec_exe, tmp_path):
    """k = 3 .. 258 moves every block cut one symbol a step against the chunk grid: bytes, state, blk_end and blk_top are the
    maps' for every k, the bytes the oracle's.  From spec_base: over the sweep a cut fell on a slab's first symbol and on a
    slab's last one (chunks of literals begin at 512 j - 262 and block b's last symbol at 16383 (b + 1) + k - 2, and
    16384 = 32 x 512: k = 252 + b .. 253 + b, inside the sweep), and random bytes fill a slab to the last symbol a chunk of 512
    positions can emit."""
    first, last, most = _sweep(engine, oracle, spec_exe, tmp_path, 512, list(range(3, 259)))
    assert first >= 1 and last >= 1, (first, last)
    assert most == 512, most


def test_a_block_cut_against_chunks_of_1024(engine, oracle, spec_exe, tmp_path):
    """The same at chunks of 1024 for every fourth k.  A cut on a slab's first or last symbol needs a lag of 763 + b .. 764 + b
    positions here (16384 = 16 x 1024), which no single match gives: a second sweep, k = 200 .. 258 with two matches of 258 behind
    it (lag k + 513), puts cuts there, and says so from spec_base."""
    first, last, most = _sweep(engine, oracle, spec_exe, tmp_path, 1024, list(range(3, 259, 4)))
    assert most == 1024, most
    first, last, most = _sweep(engine, oracle, spec_exe, tmp_path, 1024, list(range(200, 259)), more=2)
    assert first >= 1 and last >= 1, (first, last)


@pytest.mark.parametrize("level", [6, 9])
def test_few_symbols_per_slab(engine, oracle, spec_exe, tmp_path, level):
    """kennedy.xls repeated to 2 MiB: long matches, slabs of a few dozen symbols, block cuts many chunks apart.  At level 6 the
    model says it verifies, and it must here.  At level 9 (lazy 258) the model finds hundreds of wrong guesses: the walk fills its
    slabs, the verdict throws them away, and the maps' symbols must be untouched by them."""
    d = oracle_binding.corpus("kennedy.xls")
    data = d * ((2 << 20) // len(d) + 1)
    (v,) = _verdicts(spec_exe, tmp_path, [data], level, 1024)
    assert v == (level == 6), "the model's verdict on kennedy.xls changed: the case no longer proves what it says"
    bad, base, body_syms = _walk_against_maps(engine, oracle, data, level, v)
    assert not bad, bad
    if v:
        assert body_syms / len(base) < 1024 / 3


def test_a_fallback_leaves_nothing_behind(oracle):
    """One context: a walk that fails writes slabs that nobody reads, and the next calls -- the same buffer verifying, a batch in
    which one stream fails and one verifies beside a stream that never qualifies -- are what they are on their own."""
    engine = Engine(0)
    try:
        english = datagen.english(3 << 20)
        a, b, small = english[:2 << 20], english[2 << 20:3 << 20], english[5000:5000 + (100 << 10)]
        (z_maps,), _ = _deflate(engine, [a], 6, ZS_NO_SPEC=1)
        (z,), cnt = _deflate(engine, [a], 6, ZS_SPEC_CORRUPT=777)
        assert cnt == {"spec_streams": 1, "spec_fallbacks": 1, "spec_wrong_chunks": 1}, cnt
        assert z == z_maps and z == oracle.compress(a, 6)
        (z,), cnt = _deflate(engine, [a], 6)
        assert cnt == {"spec_streams": 1, "spec_fallbacks": 0, "spec_wrong_chunks": 0}, cnt
        assert z == z_maps
        single = []
        for d in (a, b, small):
            (zd,), _ = _deflate(engine, [d], 6, ZS_SPEC_LEN=1024)
            single.append(zd)
        assert engine.counter("spec_streams") == 0  # (the last of them, 100 KiB, never qualifies)
        zs, cnt = _deflate(engine, [a, b, small], 6, ZS_SPEC_LEN=1024, ZS_SPEC_CORRUPT=1500)
        # chunk 1500 exists in the 2 MiB stream only: it falls back, the 1 MiB stream verifies
        assert cnt == {"spec_streams": 2, "spec_fallbacks": 1, "spec_wrong_chunks": 1}, cnt
        assert zs == single
        assert zs[1] == oracle.compress(b, 6) and zs[2] == oracle.compress(small, 6)
    finally:
        engine.close()


def test_the_workspace_grows_and_is_used_again(oracle):
    """One fresh context: 1 MiB, then 8 MiB (every buffer of the path grows, the slabs among them), then 1 MiB in the larger
    workspace."""
    engine = Engine(0)
    try:
        english = datagen.english(8 << 20)
        for n in (1 << 20, 8 << 20, 1 << 20):
            (z,), cnt = _deflate(engine, [english[:n]], 6)
            assert cnt == {"spec_streams": 1, "spec_fallbacks": 0, "spec_wrong_chunks": 0}, (n, cnt)
            assert z == oracle.compress(english[:n], 6), n
    finally:
        engine.close()
