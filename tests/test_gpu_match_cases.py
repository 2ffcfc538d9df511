"""The encoder's front end on the device -- links (K1), match search (K2), maps and speculative walk (K3-K5), tail engine (K6), and
for levels 1-3 the sweeps, their rounds, the runs' engine and the literal engine -- on the inputs of tests/match_cases.py, byte
for byte against the oracle.  Why a case is here is its claim, which tests/test_match_cases.py holds against the oracle's stream
on the CPU; here only bytes are compared, and a claim is never evaluated on the device's stream.  Which path ran is asserted
through the engine's counters."""
import ctypes
import io
import json
import os
import subprocess
import sys
import zlib

import pytest

import match_cases as mc
from test_match_cases import ADLER_LENGTHS, ADLER_SEEDS, ref
from zlibstream_amd import CompressionLevel, ZlibOptions, ZlibOutputStream, datagen, deflate_bound

pytestmark = pytest.mark.gpu

SWITCHES = ("ZS_NO_SPEC", "ZS_SPEC_LEN", "ZS_SPEC_MIN", "ZS_FORCE_ROUNDS", "ZS_FAST_NO_ROUNDS", "ZS_FR_CHUNK", "ZS_FR_RANGE", "ZS_NO_FAST_VEC")
SPEC_COUNTERS = ("spec_streams", "spec_fallbacks", "spec_periodic", "spec_wrong_chunks")
FF_STREAM = b"\xff" * 65537  # the largest sums the trailer kernel combines: two pieces, the second one byte long


@pytest.fixture(autouse=True)
def _clean_env():
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _deflate(engine, bufs, level, strategy=0, hash_variant=0, **env):
    """one call under switches that are set for it alone"""
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return engine.deflate_batch(bufs, level=level, strategy=strategy, hash_variant=hash_variant)
    finally:
        for k in env:
            os.environ.pop(k, None)


def _groups(names):
    """the one-Write cases among `names` by (level, strategy), in catalogue order"""
    out = {}
    for n in names:
        _, _, level, strategy, writes, _ = mc.case(n)
        if writes is None:
            out.setdefault((level, strategy), []).append(n)
    return out


def _bad(oracle, names, got, level=None, strategy=None, hash_variant=0):
    return [n for n, z in zip(names, got) if z != ref(oracle, n, level, strategy, hash_variant)]


GROUPS = _groups(mc.case_names())
SLOW = sorted(k for k in GROUPS if k[0] >= 4)
FAST = sorted(k for k in GROUPS if k[0] <= 3)


def test_the_groups_cover_every_level():
    assert {k[0] for k in GROUPS} == set(range(1, 10)) and sum(len(v) for v in GROUPS.values()) == 444 - 8


@pytest.mark.parametrize("name", mc.case_names())
def test_case_alone(engine, oracle, name):
    _, data, level, strategy, writes, _ = mc.case(name)
    if writes is None:
        z = engine.deflate_batch([data], level=level, strategy=strategy)[0]
    else:
        z = _through_the_stream_api(engine, data, level, writes)
    assert z == ref(oracle, name) and zlib.decompress(z) == data


@pytest.mark.parametrize("order", ["catalogue", "reversed"])
@pytest.mark.parametrize("level,strategy", sorted(GROUPS))
def test_cases_of_a_level_in_one_batch(engine, oracle, level, strategy, order):
    """every case beside every kind of neighbour: the links, the match tiles and the tails of a batch are flat lists; an
    all-0xFF stream of 65537 bytes among them, for the trailer"""
    names = GROUPS[(level, strategy)][::-1] if order == "reversed" else GROUPS[(level, strategy)]
    got = engine.deflate_batch([mc.case(n)[1] for n in names] + [FF_STREAM], level=level, strategy=strategy)
    assert not _bad(oracle, names, got)
    assert got[-1] == oracle.compress(FF_STREAM, level, strategy) and got[-1][-4:] == zlib.adler32(FF_STREAM).to_bytes(4, "big")


# ------------------------------------------------------------------ levels 4-9: the paths
@pytest.mark.parametrize("level,strategy", SLOW)
def test_transfer_maps(engine, oracle, level, strategy):
    names = GROUPS[(level, strategy)]
    got = _deflate(engine, [mc.case(n)[1] for n in names], level, strategy, ZS_NO_SPEC=1)
    assert engine.counter("spec_streams") == 0
    assert not _bad(oracle, names, got)


_TEXT = {}


def _embedded(name):
    """the case with text behind it, so that the stream is long enough for the speculative walk: its positions stay where they are"""
    data = mc.case(name)[1]
    if "t" not in _TEXT:
        _TEXT["t"] = datagen.english(70000, 17)
    return data + _TEXT["t"][:max(0, 65536 + 777 - len(data))]


_EMBEDDED_REF = {}


@pytest.mark.parametrize("length", [512, 1024, 2048])
@pytest.mark.parametrize("level,strategy", SLOW)
def test_speculative_walk(engine, oracle, level, strategy, length):
    """ZS_SPEC_MIN=65536: every stream of the batch tries the walk.  A stream either verifies or is counted as a fallback (on the
    RUNS walk of the match kernel: periodic, never walked) and takes the maps: the counters say which, the bytes are the oracle's
    and the maps' either way."""
    names = GROUPS[(level, strategy)]
    bufs = [_embedded(n) for n in names]
    for n, d in zip(names, bufs):
        if (n, level, strategy) not in _EMBEDDED_REF:
            _EMBEDDED_REF[(n, level, strategy)] = oracle.compress(d, level, strategy)
    got = _deflate(engine, bufs, level, strategy, ZS_SPEC_MIN=65536, ZS_SPEC_LEN=length)
    cnt = {k: engine.counter(k) for k in SPEC_COUNTERS}
    print("level %d strategy %d chunks of %d: %d streams, %r" % (level, strategy, length, len(names), cnt))
    assert cnt["spec_streams"] == len(names), cnt
    assert 0 <= cnt["spec_periodic"] <= cnt["spec_fallbacks"] <= cnt["spec_streams"], cnt
    assert [n for n, z in zip(names, got) if z != _EMBEDDED_REF[(n, level, strategy)]] == [], cnt
    got0 = _deflate(engine, bufs, level, strategy, ZS_NO_SPEC=1)
    assert engine.counter("spec_streams") == 0 and got0 == got


@pytest.mark.parametrize("level,strategy", SLOW)
def test_cut_rounds(engine, oracle, level, strategy):
    names = GROUPS[(level, strategy)]
    before = engine.counter("round_runs")
    got = _deflate(engine, [mc.case(n)[1] for n in names], level, strategy, ZS_FORCE_ROUNDS=1)
    print("level %d strategy %d: round_runs + %d, cut_rounds %d" % (level, strategy, engine.counter("round_runs") - before, engine.counter("cut_rounds")))
    assert not _bad(oracle, names, got)


def test_cut_rounds_ran_for_the_equal_bucket_events(engine, oracle):
    """placement "slide_run": a run of one byte and one of two across the first window end's loop-top -- the event's loop-top shares
    its bucket with the next position, and with no cut budget that chain's cut goes to the batched rounds"""
    names = [n for n in GROUPS[(6, 0)] if n.startswith("place_slide_run_")]
    assert len(names) == 2
    before = engine.counter("round_runs")
    got = _deflate(engine, [mc.case(n)[1] for n in names], 6, ZS_FORCE_ROUNDS=1)
    assert engine.counter("round_runs") == before + 1
    assert not _bad(oracle, names, got)


@pytest.mark.parametrize("level", range(1, 10))
def test_multiplicative_hash_on_the_distance_and_budget_families(engine, oracle, level):
    names = [n for n in mc.hash_variant_names() if mc.case(n)[2] == level]
    assert names
    got = engine.deflate_batch([mc.hash_variant_case(n)[1] for n in names], level=level, hash_variant=1)
    assert not _bad(oracle, names, got, hash_variant=1)


@pytest.mark.parametrize("strategy", [mc.FILTERED, mc.HO, mc.FIXED])
def test_strategies_on_the_too_far_and_lazy_families(engine, oracle, strategy):
    names = [n for n in mc.case_names() if mc.META[n][0] in ("too_far", "max_lazy", "lazy_tie")]
    for (level, _), group in sorted(_groups(names).items()):
        got = engine.deflate_batch([mc.case(n)[1] for n in group], level=level, strategy=strategy)
        assert not _bad(oracle, group, got, level, strategy), (level, strategy)


# ------------------------------------------------------------------ levels 1-3: the paths
@pytest.mark.parametrize("level,strategy", FAST)
def test_sweeps_with_one_workgroup_per_stream(engine, oracle, level, strategy):
    names = GROUPS[(level, strategy)]
    before = engine.counter("lit_engine_bytes")
    got = _deflate(engine, [mc.case(n)[1] for n in names], level, strategy, ZS_FAST_NO_ROUNDS=1)
    assert engine.counter("fast_rounds") == 0 and engine.counter("lit_engine_bytes") == before
    assert not _bad(oracle, names, got)


@pytest.mark.parametrize("chunk", [1024, 2048])
@pytest.mark.parametrize("level,strategy", FAST)
def test_rounds_in_one_batch(engine, oracle, level, strategy, chunk):
    """(ZS_FR_CHUNK is read per call; the engine takes chunks of 2048 positions at the least, and decides by the batch's shape
    whether rounds are the shorter way: the counter is printed, the rounds are asserted in test_rounds_case_by_case)"""
    names = GROUPS[(level, strategy)]
    got = _deflate(engine, [mc.case(n)[1] for n in names], level, strategy, ZS_FR_CHUNK=chunk)
    print("level %d chunks of %d: fast_rounds %d" % (level, chunk, engine.counter("fast_rounds")))
    assert not _bad(oracle, names, got)


@pytest.mark.parametrize("fr_range", [1, 3])
def test_rounds_case_by_case(fr_range):
    """ZS_FR_RANGE is read once per process, so each value gets a process of its own (tests/match_cases_rounds.py); ZS_FR_CHUNK 1024
    and 2048 inside it.  Every one-Write case of levels 1-3 alone: its bytes, and that rounds ran."""
    env = dict(os.environ, ZS_FR_RANGE=str(fr_range))
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "match_cases_rounds.py")], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[7:])
    print("ZS_FR_RANGE=%d: %r" % (fr_range, out))
    assert out["bad"] == [] and out["calls"] == 2 * out["cases"] and out["cases"] == sum(len(GROUPS[k]) for k in FAST)
    assert out["calls_in_rounds"] >= out["calls"] // 2 and out["most_rounds"] >= 2, out


@pytest.mark.parametrize("level,strategy", FAST)
def test_literal_engine(engine, oracle, level, strategy):
    names = GROUPS[(level, strategy)]
    before = engine.counter("lit_engine_bytes")
    got = _deflate(engine, [mc.case(n)[1] for n in names], level, strategy, ZS_NO_FAST_VEC=1)
    assert engine.counter("lit_engine_bytes") - before == sum(max(0, len(mc.case(n)[1]) - 261) for n in names)  # every stream, whole
    assert not _bad(oracle, names, got)


@pytest.mark.parametrize("level", [1, 2, 3])
def test_runs_padded_to_64_kib_of_period(engine, oracle, level):
    """The run cases with their period repeated behind them up to 64 KiB and more (kFastMinPeriodic): a batch of a few such
    streams is planned for the sweeps and for the runs' engine, and the links decide.  No counter names the runs' engine; what
    the counters do say -- no sweep rounds, no batch redone sequentially -- is asserted with the bytes.  (The catalogue has its run
    cases at levels 1 and 3; level 2 takes level 1's inputs.)"""
    bufs = []
    tag = "_L%d" % (1 if level == 2 else level)
    for period, unit in ((1, b"Q"), (2, b"QR"), (3, b"QRS"), (7, b"QRSTUVW")):
        for n in [n for n in mc.case_names("runs") if n.startswith("run_p%d_" % period) and n.endswith(tag)][:3]:
            data = mc.case(n)[1]
            bufs.append(data + (unit * (70000 // period + 1))[:65536 + 3 * period + len(bufs) - len(data) % 7])
    assert 4 <= len(bufs) <= 16 and all(65536 <= len(b) < (4 << 20) for b in bufs)
    before = engine.counter("fast_fallbacks")
    got = engine.deflate_batch(bufs, level=level)
    print("level %d: %d streams, fast_rounds %d, fast_fallbacks + %d" % (level, len(bufs), engine.counter("fast_rounds"), engine.counter("fast_fallbacks") - before))
    assert engine.counter("fast_rounds") == 0 and engine.counter("fast_fallbacks") == before
    assert got == [oracle.compress(b, level) for b in bufs]


# ------------------------------------------------------------------ Write lists
def _through_the_stream_api(engine, data, level, writes):
    out = io.BytesIO()
    s = ZlibOutputStream(out, ZlibOptions(CompressionLevel=CompressionLevel(level)), engine=engine)
    at = 0
    for w in writes:
        s.write(data[at:at + w])
        at += w
    assert at == len(data)
    s.close()
    return out.getvalue()


@pytest.mark.parametrize("level", [1, 6])
def test_write_lists_through_deflate_writes_batch(engine, oracle, level):
    """the slide at a Write end: first Writes of 65400, 65534, 65535 and 65536 bytes and the single Write, one batch"""
    import torch
    names = [n for n in mc.case_names("slide") if mc.case(n)[2] == level]
    assert len(names) == 5
    ins = [torch.frombuffer(bytearray(mc.case(n)[1]), dtype=torch.uint8).cuda() for n in names]
    outs = [torch.empty(deflate_bound(t.numel()), dtype=torch.uint8, device="cuda") for t in ins]
    ends = []
    for n in names:
        writes = mc.case(n)[4]
        ends.append(None if writes is None else [sum(writes[:k + 1]) for k in range(len(writes))])
    lens = engine.deflate_writes_batch_device([t.data_ptr() for t in ins], [t.numel() for t in ins], ends, [t.data_ptr() for t in outs], [t.numel() for t in outs],
                                              level=level, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not _bad(oracle, names, [t[:m].cpu().numpy().tobytes() for t, m in zip(outs, lens)])


# ------------------------------------------------------------------ odd addresses
@pytest.mark.parametrize("level", [1, 6])
def test_inputs_at_device_pointers_of_every_residue(engine, oracle, level):
    """deflate_batch_device: the level's default-strategy batch as slices of one tensor, stream i at an address = 1 + i % 15 mod 16"""
    import torch
    names = GROUPS[(level, 0)]
    offs, at = [], 0
    for i, n in enumerate(names):
        at += (1 + i % 15 - at) % 16
        offs.append(at)
        at += len(mc.case(n)[1])
    host = bytearray(at + 16)
    for o, n in zip(offs, names):
        host[o:o + len(mc.case(n)[1])] = mc.case(n)[1]
    d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
    assert d_in.data_ptr() % 16 == 0 and {(d_in.data_ptr() + o) % 16 for o in offs} == set(range(1, 16))
    lens = [len(mc.case(n)[1]) for n in names]
    outs = [torch.empty(deflate_bound(m), dtype=torch.uint8, device="cuda") for m in lens]
    got = engine.deflate_batch_device([d_in.data_ptr() + o for o in offs], lens, [t.data_ptr() for t in outs], [t.numel() for t in outs], level=level,
                                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not _bad(oracle, names, [t[:m].cpu().numpy().tobytes() for t, m in zip(outs, got)])


# ------------------------------------------------------------------ Adler-32 at its extremes
def _device_adler(engine, ptr, n, seed):
    out = ctypes.c_uint32(0)
    assert engine._lib.zs_adler32_device(engine.handle, ctypes.c_void_p(ptr), n, seed, ctypes.byref(out), None) == 0
    return out.value


@pytest.mark.parametrize("kind", ["0xff", "random"])
def test_device_adler_lengths_seeds_and_residues(engine, kind):
    """zs_adler32_device against zlib.adler32(data, seed): all-0xFF buffers (the largest sums the piece kernel's 64-bit lanes and
    adler_combine see) and random ones (an all-equal buffer cannot show bytes out of place); 0 bytes to 256 pieces and one byte
    (`per` = 2 in the finish kernel); every seed; the buffer at every residue mod 16 (the 16-byte path is taken only where
    p + o is aligned)."""
    import random
    import torch
    big = ADLER_LENGTHS[-1]
    host = b"\xff" * (big + 16) if kind == "0xff" else random.Random(5).randbytes(big + 16)
    t = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    bad = []
    for n in ADLER_LENGTHS:
        for r in range(16):
            want1 = zlib.adler32(host[r:r + n])
            for seed in ADLER_SEEDS if (r < 2 or n < big) else ADLER_SEEDS[:1]:
                got = _device_adler(engine, t.data_ptr() + r, n, seed)
                if got != zlib.adler32(host[r:r + n], seed) or (seed == 1 and got != want1):
                    bad.append((n, r, seed, got))
    assert not bad, bad[:10]
