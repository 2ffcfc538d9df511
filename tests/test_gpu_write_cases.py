"""The read schedule on the device -- the host's geometry and read events, the kernels' event prefix (chunk_special_prefix), the
sweeps' events, the literal engine and the router between them -- on the Write lists of tests/write_cases.py, byte for byte
against the oracle's stream of the same schedule.  Why a case is here is its claim, which tests/test_write_cases.py holds against
the oracle's trace on the CPU; here only bytes are compared, and a claim is never evaluated on the device's stream.  Which path
ran is asserted through the engine's counters."""
import io
import os
import zlib

import pytest

import match_cases as mc
import write_cases as wc
from write_cases import ref, single
from zlibstream_amd import CompressionLevel, CompressionStrategy, Engine, FlushMode, ZlibOptions, ZlibOutputStream, deflate_bound

pytestmark = pytest.mark.gpu

SWITCHES = ("ZS_NO_SPEC", "ZS_SPEC_LEN", "ZS_SPEC_MIN", "ZS_FORCE_ROUNDS", "ZS_FAST_NO_ROUNDS", "ZS_FR_CHUNK", "ZS_NO_FAST_VEC")


@pytest.fixture(autouse=True)
def _clean_env():
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _deflate(engine, datas, ends, level, strategy=0, hash_variant=0, **env):
    """one zs_deflate_writes_batch_device call on fresh device buffers, under switches that are set for it alone"""
    import torch
    d_in = [torch.frombuffer(bytearray(d) + bytearray(64), dtype=torch.uint8).cuda() for d in datas]
    caps = [deflate_bound(len(d)) for d in datas]
    d_out = [torch.full((c + 64,), 0xEE, dtype=torch.uint8, device="cuda") for c in caps]
    torch.cuda.synchronize()
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        lens = engine.deflate_writes_batch_device([t.data_ptr() for t in d_in], [len(d) for d in datas], ends, [t.data_ptr() for t in d_out], caps, level=level,
                                                  strategy=strategy, hash_variant=hash_variant)
    finally:
        for k in env:
            os.environ.pop(k, None)
    return [bytes(t[:n].cpu().numpy()) for t, n in zip(d_out, lens)]


def _groups():
    """the catalogue's NoFlush cases by (level, strategy), in catalogue order (the resume family goes through the stream classes)"""
    out = {}
    for n in NOFLUSH:
        _, _, level, strategy, _, _, _, _ = wc.case(n)
        out.setdefault((level, strategy), []).append(n)
    return out


NOFLUSH = [n for n in wc.case_names() if wc.META[n][0] != "resume"]
RESUME = wc.case_names("resume")
GROUPS = _groups()
SLOW = sorted(k for k in GROUPS if k[0] >= 4 and k[1] != mc.RLE)
FAST = sorted(k for k in GROUPS if k[0] <= 3 and k[1] != mc.RLE)


def _batch(names, reverse=False):
    """The cases and, among them, their bytes as one Write (once per distinct input): (datas, ends, the oracle's name per stream).
    A name with a trailing "|1" stands for the single Write's stream."""
    datas, ends, who, seen = [], [], [], set()
    for n in names[::-1] if reverse else names:
        _, data, _, _, e, _, _, _ = wc.case(n)
        datas.append(data), ends.append(e), who.append(n)
        if data not in seen:
            seen.add(data)
            datas.append(data), ends.append(None), who.append(n + "|1")
    return datas, ends, who


def _want(oracle, who):
    return single(oracle, who[:-2]) if who.endswith("|1") else ref(oracle, who)


def _bad(oracle, who, got):
    return [w for w, z in zip(who, got) if z != _want(oracle, w)]


def test_the_groups_cover_the_catalogue():
    assert sum(len(v) for v in GROUPS.values()) == 182 - 22 == len(NOFLUSH) and len(RESUME) == 22 and {k[0] for k in GROUPS} == {1, 2, 3, 4, 6, 9}


# ------------------------------------------------------------------ alone, batched, through the stream classes
CUMULATIVE = ("lit_engine_bytes", "lit_fallbacks", "round_runs", "fast_fallbacks")


def _alone(engine, data, level, strategy, ends):
    """zs_deflate_writes_device: (stream, what the cumulative counters grew by, fast_rounds of the call)"""
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = torch.empty(deflate_bound(len(data)), dtype=torch.uint8, device="cuda")
    before = [engine.counter(k) for k in CUMULATIVE]
    n = engine.deflate_writes_device(t.data_ptr(), len(data), ends, out.data_ptr(), out.numel(), level=level, strategy=strategy)
    return bytes(out[:n].cpu().numpy()), dict(zip(CUMULATIVE, [engine.counter(k) - b for k, b in zip(CUMULATIVE, before)])), engine.counter("fast_rounds")


@pytest.mark.parametrize("name", NOFLUSH)
def test_case_alone(engine, oracle, name):
    """zs_deflate_writes_device, and the path the planner chose, through the counters around the call"""
    _, data, level, strategy, ends, _, _, route = wc.case(name)
    z, grew, rounds = _alone(engine, data, level, strategy, ends)
    lit, fallbacks = grew["lit_engine_bytes"], grew["lit_fallbacks"]
    assert z == ref(oracle, name) and zlib.decompress(z) == data
    if route == "literal":
        assert (lit, fallbacks) == (len(data) - 261, 0)
    elif route == "poisoned":
        assert fallbacks == 1
    else:
        assert (lit, fallbacks) == (0, 0), route
    if route == "folded":  # the call is the single Write's in every counter: its bytes (held on the CPU), its path
        z1, grew1, rounds1 = _alone(engine, data, level, strategy, [len(data)])
        assert (z1, grew1, rounds1) == (z, grew, rounds)


def _flushed_stream(engine, data, level, strategy, ends, flushes):
    """ZlibOptions.FlushMode is read by every Write: set anew before each"""
    out = io.BytesIO()
    s = ZlibOutputStream(out, ZlibOptions(CompressionLevel=CompressionLevel(level), CompressionStrategy=CompressionStrategy(strategy), FlushMode=FlushMode(0)),
                         engine=engine)
    at = 0
    for e, f in zip(ends, flushes):
        s.Options.FlushMode = FlushMode(f)
        s.write(data[at:e])
        at = e
    s.Options.FlushMode = FlushMode(0)
    s.close()
    return out.getvalue()


@pytest.mark.parametrize("name", RESUME)
def test_resume_case_through_the_stream_classes(engine, oracle, name):
    """The first Write under its flush mode, the others under NoFlush, Finish: the run behind the flush goes on in the parallel
    forms from the flush itself (GeoStart::at_read, on the chains the first run's engine left) or stays with the literal engine,
    which then parses all that lies behind the flush."""
    _, data, level, strategy, ends, flushes, _, route = wc.case(name)
    lit = engine.counter("lit_engine_bytes")
    z = _flushed_stream(engine, data, level, strategy, ends, flushes)
    lit = engine.counter("lit_engine_bytes") - lit
    print("%s: lit_engine_bytes + %d (flush at %d of %d, %s)" % (name, lit, ends[0], len(data), route))
    assert z == ref(oracle, name) and zlib.decompress(z) == data
    # (the flushed Write itself is a bulk run with the tail engine left suspended: nothing for the literal engine.  The stream
    # classes hand a run to the planner from kResumeMinBytes = 1 KiB on: the runs of 524 bytes, which the planner would take --
    # tests/test_write_cases.py holds that on the host -- stay with the literal engine like those of 523.)
    behind = len(data) - ends[0]
    assert lit == (0 if route == "resumed" and behind >= 1024 else behind - 261), (lit, route)


@pytest.mark.parametrize("order", ["catalogue", "reversed"])
@pytest.mark.parametrize("level,strategy", sorted(GROUPS))
def test_cases_of_a_level_in_one_batch(engine, oracle, level, strategy, order):
    """every case beside every kind of neighbour, its own bytes as a single Write among them: segment tables, cluster lists and
    cut slots of a batch are flat lists.  A poisoned stream sends the whole batch round again: the others stay exact."""
    datas, ends, who = _batch(GROUPS[(level, strategy)], order == "reversed")
    fallbacks = engine.counter("lit_fallbacks")
    got = _deflate(engine, datas, ends, level, strategy)
    assert not _bad(oracle, who, got)
    poisoned = sum(wc.case(n)[7] == "poisoned" for n in GROUPS[(level, strategy)])
    assert engine.counter("lit_fallbacks") - fallbacks == (1 if poisoned else 0)


def _through_the_stream_api(engine, data, level, strategy, ends):
    out = io.BytesIO()
    s = ZlibOutputStream(out, ZlibOptions(CompressionLevel=CompressionLevel(level), CompressionStrategy=CompressionStrategy(strategy)), engine=engine)
    at = 0
    for e in ends:
        s.write(data[at:e])
        at = e
    s.close()
    return out.getvalue()


@pytest.mark.parametrize("name", [n for k in sorted(GROUPS) if k[0] in (1, 6) for n in GROUPS[k]])
def test_case_through_the_stream_classes(engine, oracle, name):
    _, data, level, strategy, ends, _, _, _ = wc.case(name)
    assert _through_the_stream_api(engine, data, level, strategy, ends) == ref(oracle, name)


# ------------------------------------------------------------------ levels 4-9: the paths
@pytest.mark.parametrize("level,strategy", SLOW)
def test_transfer_maps(engine, oracle, level, strategy):
    datas, ends, who = _batch(GROUPS[(level, strategy)])
    got = _deflate(engine, datas, ends, level, strategy, ZS_NO_SPEC=1)
    assert engine.counter("spec_streams") == 0
    assert not _bad(oracle, who, got)


@pytest.mark.parametrize("length", [512, 2048])
@pytest.mark.parametrize("level,strategy", SLOW)
def test_speculative_walk_beside_the_write_lists(engine, oracle, level, strategy, length):
    """ZS_SPEC_MIN=65536: every stream without a Write list (the walk takes a single Write alone) of 64 KiB or more tries the
    walk, in one batch with the Write lists on the maps"""
    datas, ends, who = _batch(GROUPS[(level, strategy)])
    got = _deflate(engine, datas, ends, level, strategy, ZS_SPEC_MIN=65536, ZS_SPEC_LEN=length)
    assert engine.counter("spec_streams") == sum(e is None and len(d) >= 65536 for d, e in zip(datas, ends)) > 0
    assert not _bad(oracle, who, got)


@pytest.mark.parametrize("level,strategy", SLOW)
def test_cut_rounds(engine, oracle, level, strategy):
    """ZS_FORCE_ROUNDS=1: no cut on the stream's own CU, the batched rounds from the first cut on.  A chain is cut where an event
    loop-top shares its bucket with the next position (the eq_bucket cases of period 1): a level that has those runs the rounds."""
    names = GROUPS[(level, strategy)]
    datas, ends, who = _batch(names)
    before = engine.counter("round_runs")
    got = _deflate(engine, datas, ends, level, strategy, ZS_FORCE_ROUNDS=1)
    grown = engine.counter("round_runs") - before
    print("level %d: round_runs + %d, cut_rounds %d" % (level, grown, engine.counter("cut_rounds")))
    assert grown == (1 if any(wc.META[n][1].startswith("eq_bucket") and wc.META[n][2] == "in" for n in names) else 0)
    assert not _bad(oracle, who, got)


# ------------------------------------------------------------------ levels 1-3: the paths
@pytest.mark.parametrize("level,strategy", FAST)
def test_sweeps_with_one_workgroup_per_stream(engine, oracle, level, strategy):
    datas, ends, who = _batch(GROUPS[(level, strategy)])
    got = _deflate(engine, datas, ends, level, strategy, ZS_FAST_NO_ROUNDS=1)
    assert engine.counter("fast_rounds") == 0
    assert not _bad(oracle, who, got)


@pytest.mark.parametrize("chunk", [1024, 2048])
@pytest.mark.parametrize("level,strategy", FAST)
def test_rounds_in_one_batch(engine, oracle, level, strategy, chunk):
    datas, ends, who = _batch(GROUPS[(level, strategy)])
    got = _deflate(engine, datas, ends, level, strategy, ZS_FR_CHUNK=chunk)
    print("level %d chunks of %d: fast_rounds %d" % (level, chunk, engine.counter("fast_rounds")))
    assert not _bad(oracle, who, got)


@pytest.mark.parametrize("chunk", [1024, 2048])
@pytest.mark.parametrize("level,strategy", FAST)
def test_rounds_case_by_case(engine, oracle, level, strategy, chunk):
    """A batch of many short streams takes one workgroup per stream, so the rounds are asked for case by case: a Write list on the
    sweeps' route alone in its call runs as rounds over its chunks, the events applied where a chunk's sweep starts -- unless two
    of its data ends are less than kFsMinSpan = 520 apart (chunks are cut at the events: zs_plan.h plan_fast_rounds, too_short);
    one on the literal route does not."""
    bad, in_rounds = [], 0
    for name in GROUPS[(level, strategy)]:
        _, data, _, _, ends, _, _, route = wc.case(name)
        if len(ends) == 1:
            continue  # (the length cases: one Write, one chunk)
        (z,) = _deflate(engine, [data], [ends], level, strategy, ZS_FR_CHUNK=chunk)
        rounds = engine.counter("fast_rounds")
        b = [0] + wc.read_ends(len(data), ends)[:-1]
        want_rounds = route == "sweeps" and min(y - x for x, y in zip(b, b[1:])) >= 520
        in_rounds += rounds > 0
        if z != ref(oracle, name) or (rounds > 0) != want_rounds:
            bad.append((name, rounds, want_rounds))
    print("level %d chunks of %d: %d of %d Write lists ran as rounds" % (level, chunk, in_rounds, len(GROUPS[(level, strategy)])))
    assert not bad, bad
    assert in_rounds >= 2


@pytest.mark.parametrize("level,strategy", FAST)
def test_literal_engine(engine, oracle, level, strategy):
    datas, ends, who = _batch(GROUPS[(level, strategy)])
    before = engine.counter("lit_engine_bytes")
    got = _deflate(engine, datas, ends, level, strategy, ZS_NO_FAST_VEC=1)
    assert engine.counter("lit_engine_bytes") - before == sum(max(0, len(d) - 261) for d in datas)  # every stream, whole
    assert not _bad(oracle, who, got)


# ------------------------------------------------------------------ the multiplicative hash
@pytest.mark.parametrize("level", [1, 3, 4, 6, 9])
def test_multiplicative_hash_on_the_event_top_and_slide_families(engine, oracle, level):
    names = [n for n in wc.hash_variant_names() if wc.case(n)[2] == level]
    assert names
    got = _deflate(engine, [wc.case(n)[1] for n in names], [wc.case(n)[4] for n in names], level, hash_variant=1)
    want = [oracle.compress(wc.case(n)[1], level, 0, chunks=wc.writes(wc.case(n)[4]), hash_variant=1) for n in names]
    assert [n for n, z, w in zip(names, got, want) if z != w] == []


# ------------------------------------------------------------------ plan reuse
PLAN_TWINS = (("top_behind_match_L6", "top_on_b261_L6"), ("ahead_261_L6", "ahead_262_L6"), ("gap_270_L6", "gap_271_L6"), ("slide_end_65534_L6", "slide_end_65535_L6"),
              ("tail_last_at_524_L6", "tail_last_at_523_L6"), ("poison_six_ahead_L9", "poison_seven_ahead_L9"), ("fast_read_262_L1", "fast_read_261_L1"),
              ("rle_end_65273_L6", "rle_end_65274_L6"))


@pytest.fixture(scope="module")
def own_engine():
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("a,b", PLAN_TWINS, ids=[p[0] for p in PLAN_TWINS])
def test_twins_do_not_share_a_plan(own_engine, oracle, a, b):
    """Twins have the same length, level and capacity and differ in one Write end: side A, side B, side B with other bytes of its
    shape.  The kept plan is keyed by the Write list: plan_reused reads 0, 0, 1, and every output is the oracle's."""
    _, da, level, strategy, ea, _, _, _ = wc.case(a)
    _, db, _, _, eb, _, _, _ = wc.case(b)
    other = wc.case(b, 7)[1]
    assert len(da) == len(db) == len(other) and other != db and ea != eb and wc.META[a][0] == wc.META[b][0]
    reused = []
    for name, data, ends in ((a, da, ea), (b, db, eb), (None, other, eb)):
        (z,) = _deflate(own_engine, [data], [ends], level, strategy)
        reused.append(own_engine.counter("plan_reused"))
        assert z == (ref(oracle, name) if name else oracle.compress(other, level, strategy, chunks=wc.writes(eb)))
    assert reused == [0, 0, 1]
