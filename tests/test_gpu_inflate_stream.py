"""zs_inflate piece by piece on the device: the catalogue of tests/inflate_stream_cases.py (tests/test_inflate_stream_cases.py
holds its claims) fed by schedule through the C entry points, every call's return code, bytes taken, bytes given, adler,
total_in and total_out compared exactly with the protocol's model (inflate_stream_cases.expect) -- every cut of a small
stream, two and three cuts, 300 resumes at every bit phase, histories of every size, the ring's wrap, a full output buffer,
matches one byte too far, errors in a resumed piece, output drained byte by byte, bytes behind the trailer, and the
buffering threshold in a process of its own."""
import ctypes
import os
import random
import subprocess
import sys
import zlib

import pytest

import deflate_reader as dr
import inflate_bad_cases as bc
import inflate_stream_cases as sc
from inflate_stream_cases import ROOM, ZS_BUF_ERROR, ZS_DATA_ERROR, ZS_OK, ZS_STREAM_END

pytestmark = pytest.mark.gpu

GUARD = 64
_OUT = ctypes.create_string_buffer(ROOM + GUARD)
OBJECTS = [0]  # stream objects made so far (the tests print their share)


class Stream:
    """One zs_inflate_stream and the table of its calls: (rc, taken, given, adler, total_in, total_out)."""

    def __init__(self, engine):
        self.lib = engine._lib
        self.z = self.lib.zs_inflate_init(engine.handle, 15)
        assert self.z
        self.calls = []
        self.adler, self.total_in, self.total_out = ctypes.c_uint32(1), ctypes.c_int64(0), ctypes.c_int64(0)
        OBJECTS[0] += 1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.zs_inflate_end(self.z)
        self.z = None

    def call(self, data, room):
        assert 0 <= room <= ROOM
        src = ctypes.create_string_buffer(bytes(data), max(1, len(data)))
        avail_in, avail_out = ctypes.c_int32(len(data)), ctypes.c_int32(room)
        ctypes.memset(ctypes.addressof(_OUT) + room, 0xEE, GUARD)
        rc = self.lib.zs_inflate(self.z, ctypes.cast(src, ctypes.c_void_p), ctypes.byref(avail_in), ctypes.cast(_OUT, ctypes.c_void_p),
                                 ctypes.byref(avail_out), 0, ctypes.byref(self.adler), ctypes.byref(self.total_in), ctypes.byref(self.total_out))
        assert 0 <= avail_in.value <= len(data) and 0 <= avail_out.value <= room
        assert ctypes.string_at(ctypes.addressof(_OUT) + room, GUARD) == b"\xee" * GUARD, "bytes written behind avail_out"
        row = (rc, len(data) - avail_in.value, ctypes.string_at(_OUT, room - avail_out.value), self.adler.value, self.total_in.value,
               self.total_out.value)
        self.calls.append(row)
        return row

    def message(self):
        return (self.lib.zs_inflate_message(self.z) or b"").decode()

    def surplus(self):
        p = ctypes.c_void_p()
        n = self.lib.zs_inflate_surplus(self.z, ctypes.byref(p))
        return ctypes.string_at(p, n) if n else b""

    def run(self, data, schedule):
        """The schedule's steps over `data`; a step brings the bytes behind those taken so far."""
        pos = 0
        for nbytes, room in schedule:
            row = self.call(data[pos:pos + nbytes], room)
            pos += row[1]
        return pos


def table(s, last=12):
    return [(rc, taken, len(given), "%08x" % adler, tin, tout) for rc, taken, given, adler, tin, tout in s.calls[-last:]]


def check(engine, c, schedule, tail=b"", extra=b""):
    """Run the schedule on a fresh stream object and compare every call with the model; returns the object's surplus.
    After every call total_out is what was given, total_in what was taken (the stream's length once it is through), and
    whenever everything decoded has been read adler is the plaintext's so far."""
    want, want_surplus = sc.expect(c, schedule, tail)
    data = c.z + tail + extra
    with Stream(engine) as s:
        pos = given = 0
        for k, ((nbytes, room), (rc, taken, part)) in enumerate(zip(schedule, want)):
            row = s.call(data[pos:pos + nbytes], room)
            where = (c.name, k, (nbytes, room), table(s))
            assert row[0] == rc and row[1] == taken, where
            assert row[2] == part, where + (len(part),)
            pos += taken
            given += len(part)
            through = ZS_STREAM_END in [r[0] for r in s.calls]
            assert row[5] == given and row[4] == (len(c.z) if through else pos), where
            if rc == ZS_BUF_ERROR:
                assert s.message() == "buffer error", where
            if not sc.is_bad(c) and given == sc.delivered(c, min(pos, len(c.z))) and (through or pos <= len(c.z)):
                assert row[3] == zlib.adler32(c.plain[:given]), where
        got = b"".join(r[2] for r in s.calls)
        if want and want[-1][0] == ZS_STREAM_END:
            assert got == c.plain and s.total_in.value == len(c.z) and s.total_out.value == len(c.plain)
            assert s.adler.value == zlib.adler32(c.plain)
            if c.blocks[-1][3] > (c.blocks[-2][3] if len(c.blocks) > 1 else 0):  # ZS_STREAM_END comes with the last byte
                assert [r[0] for r in s.calls].index(ZS_STREAM_END) == max(i for i, r in enumerate(s.calls) if r[2])
            assert s.surplus() == want_surplus, (c.name, len(s.surplus()), len(want_surplus))
        return s.surplus(), pos, list(s.calls)


def after_the_end(n):
    """Two more calls for a stream that has ended: one without input, one that brings bytes (they stay with the caller)."""
    return [(0, ROOM), (n, ROOM)]


# ------------------------------------------------------------------ every cut
@pytest.mark.parametrize("part", range(4))
def test_every_cut_of_mixed_small(engine, part):
    """n = 0 .. len(z): feed z[:n], ask without input (exactly plaintext[:delivered(n)]; ZS_BUF_ERROR "buffer error" when that
    is nothing), feed the rest, ask until ZS_STREAM_END, which comes with the last byte; one more call, with input, is
    ZS_STREAM_END again and takes nothing.  (part: n mod 4.)"""
    c = sc.case("mixed_small")
    before = OBJECTS[0]
    for n in range(part, len(c.z) + 1, 4):
        check(engine, c, sc.cut_schedule(len(c.z), [n]) + after_the_end(5), extra=b"EXTRA")
    print("every cut of mixed_small, part %d: %d stream objects" % (part, OBJECTS[0] - before))


def probe_cuts():
    c = sc.case("mixed_probe")
    cuts = {e + d for e in sc.block_ends(c) for d in range(-2, 3)} | set(bc.sweep_single_cuts()) | {len(c.z) - k for k in range(5)}
    return sorted(n for n in cuts if 0 <= n <= len(c.z))


def test_cuts_of_mixed_probe(engine):
    """A stream above 1 KiB: a call without input looks for the end first (finder, measuring pass, chain) and falls to the
    piece.  Cuts within 2 bytes of every block end, at inflate_bad_cases.sweep_single_cuts() and inside the trailer."""
    c = sc.case("mixed_probe")
    before = OBJECTS[0]
    for n in probe_cuts():
        check(engine, c, sc.cut_schedule(len(c.z), [n]) + after_the_end(5), extra=b"EXTRA")
    print("cuts of mixed_probe: %d stream objects" % (OBJECTS[0] - before))


@pytest.mark.parametrize("cuts", [2, 3])
def test_two_and_three_cuts_of_mixed_small(engine, cuts):
    """200 seeded pairs (triples) of cut points, a call without input at each: the bytes behind the k-th call are
    plaintext[delivered(n_(k-1)):delivered(n_k)]."""
    c = sc.case("mixed_small")
    rng = random.Random(400 + cuts)
    before = OBJECTS[0]
    for _ in range(200):
        ns = sorted(rng.randint(0, len(c.z)) for _ in range(cuts))
        _, _, calls = check(engine, c, sc.cut_schedule(len(c.z), ns))
        asked = [r for r in calls if r[1] == 0]
        edges = [0] + [sc.delivered(c, n) for n in ns] + [len(c.plain)]
        assert [r[2] for r in asked[:cuts + 1]] == [c.plain[a:b] for a, b in zip(edges, edges[1:])], ns
    print("%d cuts of mixed_small: %d stream objects" % (cuts, OBJECTS[0] - before))


def test_tiny_phases_300_resumes(engine):
    """One stream object, a cut behind each of 300 small blocks: every piece but the first is a resumed one, and every bit
    phase is resumed from at least 20 times."""
    c = sc.case("tiny_phases")
    phases = [sc.resume_phase(c, n) for n in c.info["cuts"]]
    counts = [phases.count(p) for p in range(8)]
    assert len(phases) == 300 and min(counts) >= 20, counts
    before = OBJECTS[0]
    _, _, calls = check(engine, c, list(c.schedule) + after_the_end(3), extra=b"xyz")
    assert sum(1 for r in calls if r[1] == 0 and r[2]) >= 300
    print("tiny_phases: %d stream object, resumes per bit phase 0..7: %s" % (OBJECTS[0] - before, counts))


# ------------------------------------------------------------------ histories, the ring, a full output
@pytest.mark.parametrize("name", [n for n in sc.case_names() if n.startswith("hist_edges")])
def test_hist_edges(engine, name):
    """A resumed piece whose first token reaches the oldest byte of a history of 1, 257, 32767 and 32768 bytes (and of 32768
    out of 32769 and 40000), the history taken from one piece or assembled from many; cut at the boundary and a byte either
    side."""
    c = sc.case(name)
    before = OBJECTS[0]
    for d in (-1, 0, 1):
        check(engine, c, sc.cut_schedule(len(c.z), c.info["cuts"][:-1] + [c.info["cut"] + d]))
    print("%s: %d stream objects" % (name, OBJECTS[0] - before))


@pytest.mark.parametrize("name", ["ring_wrap", "ring_wrap_stored"])
def test_ring_wrap(engine, name):
    """A resumed piece of 200 KiB: matches of distance 32768 and a stored block across the ring's wrap and its middle."""
    c = sc.case(name)
    check(engine, c, c.schedule)
    print("%s: 1 stream object" % name)


def test_full_output_stops_between_blocks(engine):
    """A piece whose output buffer is full behind a complete block stops there without an error: every call without input
    gives a whole number of blocks, the first at least one and not all.  Its twin's one block fits no first buffer: the host
    grows it and the call gives 3 MiB."""
    c = sc.case("full_output")
    ends = [blk[3] for blk in c.blocks]
    with Stream(engine) as s:
        assert s.call(c.z[:-1], ROOM)[:3] == (ZS_OK, len(c.z) - 1, b"")
        given, gives = 0, []
        while True:
            rc, taken, part = s.call(b"", ROOM)[:3]
            if rc == ZS_BUF_ERROR:
                break
            assert rc == ZS_OK and taken == 0 and part == c.plain[given:given + len(part)], table(s)
            given += len(part)
            gives.append(ends.index(given))  # (a block end, or this raises)
            assert s.adler.value == zlib.adler32(c.plain[:given]) and s.total_out.value == given
            assert len(gives) <= 6
        assert s.message() == "buffer error" and not part
        assert 0 <= gives[0] < 5 and gives[-1] == 5 and gives == sorted(set(gives)), gives  # block 5 is the last non-final one
        assert s.call(c.z[-1:], ROOM)[:3] == (ZS_OK, 1, b"")
        assert s.call(b"", ROOM)[:3] == (ZS_STREAM_END, 0, c.plain[given:])
        assert (s.adler.value, s.total_in.value, s.total_out.value) == (zlib.adler32(c.plain), len(c.z), len(c.plain))
    print("full_output: 1 stream object, blocks complete behind each call without input: %s" % [g + 1 for g in gives])
    t = sc.case("full_output_twin")
    _, _, calls = check(engine, t, t.schedule)
    assert len(calls[1][2]) == 3 << 20
    print("full_output_twin: 1 stream object")


# ------------------------------------------------------------------ errors
def batch_message(engine, z, cap):
    from zlibstream_amd import ZlibStreamException
    with pytest.raises(ZlibStreamException) as e:
        engine.inflate_batch([z], [cap])
    assert str(e.value).startswith("inflating: ")
    return str(e.value)[len("inflating: "):]


@pytest.mark.parametrize("h", sc.TOO_FAR_SIZES)
def test_too_far(engine, h):
    """A match one byte further than the stream has bytes, as the first token of a resumed piece: the first call gives the
    first part, the next is ZS_DATA_ERROR "invalid distance code", and so is the same call again.  The same stream uncut
    fails in the first piece with the message the batch call has for it and gives nothing.  The twin whose match reaches
    the first byte exactly decodes."""
    c = sc.case("too_far_%d" % h)
    want = batch_message(engine, c.z, h + 300)
    assert want == "invalid distance code"
    before = OBJECTS[0]
    for name in ("too_far_%d" % h, "too_far_%d_uncut" % h):
        c = sc.case(name)
        steps = list(c.schedule) + [(0, ROOM)]  # the failing call once more
        model, _ = sc.expect(c, steps)
        assert [m[0] for m in model[-2:]] == [ZS_DATA_ERROR] * 2
        with Stream(engine) as s:
            s.run(c.z, steps)
            assert [(r[0], r[1], r[2]) for r in s.calls] == model, (name, table(s))
            assert s.message() == want
            got = b"".join(r[2] for r in s.calls)
            assert got == (b"" if name.endswith("uncut") else c.plain) and len(got) in [0] + [blk[3] for blk in c.blocks]
            assert s.total_out.value == len(got) and s.total_in.value == len(c.z)
    legal = sc.case("too_far_%d_legal" % h)
    check(engine, legal, sc.cut_schedule(len(legal.z), [legal.info["cut"]]))
    print("too_far_%d: %d stream objects" % (h, OBJECTS[0] - before))


@pytest.mark.parametrize("name", ["hlit_287_behind_100k", "fixed_lit_286_behind_100k", "nlen_bit_8_behind_100k"])
def test_error_in_a_resumed_piece(engine, name):
    """One case of each class of inflate_bad_cases -- a block header, symbols, a stored block's lengths -- behind 100 000 bytes:
    fed up to the end of the second block (the whole stream is under 7 KB; that block end has 34 KB of plaintext, above 10 KB,
    between it and the damage), asked, fed the rest, asked: the batch call's code and message, and what was given before is the
    plaintext up to that block end."""
    _, z, rc, message, _, prefix = bc.case(name)
    head = bc._prefix_builder("behind_100k")
    cut = (head.blocks[1][1] + head.blocks[1][2] + 7) // 8
    plain_at_cut = len(zlib.decompressobj().decompress(z[:cut]))  # (zlib may be some tokens into the third block)
    assert z[:cut] == bytes(head.buf[:cut]) and 10000 <= len(prefix) - plain_at_cut
    assert batch_message(engine, z, bc.capacity(bc.case(name))) == message
    rd = dr.read(bc.case("btype_1_behind_100k")[1])  # (the same three blocks in front of a legal end)
    first, one_less = len(dr.replay(rd[:2])), len(dr.replay(rd[:1]))
    assert one_less < first <= plain_at_cut
    with Stream(engine) as s:
        assert s.call(z[:cut], ROOM)[:3] == (ZS_OK, cut, b"")
        r = s.call(b"", ROOM)
        assert r[0] == ZS_OK and r[2] == prefix[:first], table(s)
        assert r[3] == zlib.adler32(prefix[:first])
        assert s.call(z[cut:], ROOM)[:3] == (ZS_OK, len(z) - cut, b"")
        for _ in range(2):
            assert s.call(b"", ROOM)[:3] == (rc, 0, b"") and s.message() == message, table(s)
        assert s.total_out.value == first and s.total_in.value == len(z)
    # the block end: a stream object of its own, cut one byte earlier, gives a block less
    with Stream(engine) as s:
        s.call(z[:cut - 1], ROOM)
        assert s.call(b"", ROOM)[2] == prefix[:one_less]
    print("%s: 2 stream objects" % name)


# ------------------------------------------------------------------ draining
@pytest.mark.parametrize("room", [1, 2, 3, 255, 70000])
def test_draining(engine, room):
    """mixed_small read avail_out bytes at a time behind three cuts: a piece's end falls inside, at or behind a read.  A call
    with *avail_out == 0 and no input is ZS_BUF_ERROR and loses nothing, before a piece is decoded and in the middle of one;
    a call that brings input while a piece waits to be read leaves the input with the caller and serves output."""
    c = sc.case("mixed_small")
    ends = sc.block_ends(c)
    cuts = [ends[0], ends[len(ends) // 2], ends[-2], len(c.z)]
    steps, at, given = [], 0, 0
    for n in cuts:
        steps += [(n - at, room), (0, 0)]           # feed; no room: the piece is decoded and kept
        at = n
        left = sc.delivered(c, n) - given
        given += left
        reads = -(-left // room)
        for k in range(reads):
            if k == 1:
                steps += [(0, 0), (7, room)]        # in the middle of a piece: no room; input that has to wait (it serves)
            else:
                steps.append((0, room))
        if n < len(c.z):
            steps.append((0, room))                 # behind the piece: nothing new
    steps += after_the_end(4)
    want, _ = sc.expect(c, steps)
    assert [w[0] for w in want if w[0] != ZS_OK].count(ZS_BUF_ERROR) >= 7 and want[-1][0] == ZS_STREAM_END
    check(engine, c, steps, extra=b"WAIT" * 4)
    print("draining by %d: 1 stream object, %d calls" % (room, len(steps)))


# ------------------------------------------------------------------ behind the trailer
@pytest.mark.parametrize("t", [1, 4, 5000])
def test_bytes_behind_the_trailer(engine, t):
    """(a) stream and tail in one call, (b) the tail in a call of its own, (c) resumed pieces, the tail brought with the trailer's
    last byte: the call without input that meets the end leaves *avail_in at 0, the tail is zs_inflate_surplus, total_in the
    stream's length.  mixed_small ends in a piece, mixed_probe (above 1 KiB) in the whole-stream decoder."""
    tail = random.Random(410 + t).randbytes(t)
    before = OBJECTS[0]
    for name in ("mixed_small", "mixed_probe", "hist_edges_257_many"):
        c = sc.case(name)
        n = len(c.z)
        mid = sc.block_ends(c)[len(c.blocks) // 2]
        for label, steps in (("a", [(n + t, ROOM), (0, ROOM)]), ("b", [(n, ROOM), (t, ROOM), (0, ROOM)]),
                             ("c", [(mid, ROOM), (0, ROOM), (n - 1 - mid, ROOM), (0, ROOM), (1 + t, ROOM), (0, ROOM)])):
            surplus, pos, calls = check(engine, c, steps + after_the_end(2), tail=tail, extra=b"zz")
            assert surplus == tail and pos == n + t and calls[-3][0] == ZS_STREAM_END and calls[-3][4] == n, (name, label)
    print("behind the trailer, %d bytes: %d stream objects" % (t, OBJECTS[0] - before))


@pytest.mark.parametrize("name", ["mixed_probe", "hist_edges_32768_one"])
def test_cut_inside_the_trailer(engine, name):
    """1, 2 and 3 bytes of the trailer hold the final block back; it comes, with ZS_STREAM_END, when the rest does."""
    c = sc.case(name)
    for k in (1, 2, 3):
        n = len(c.z) - 4 + k
        assert sc.delivered(c, n) == c.blocks[-2][3] < len(c.plain)
        check(engine, c, sc.cut_schedule(len(c.z), [n]))
    print("%s cut inside the trailer: 3 stream objects" % name)


def test_end_found_by_a_call_that_brings_the_tail(engine):
    """A stream above 1 MiB of compressed bytes.  The first call (1.1 MB) has the end looked for, in vain; the next look is at
    four times that.  (1) The rest of the stream and 5000 bytes behind it come in a call below that mark, the look is made
    by a third call that brings only bytes behind the end: all of them stay with the caller, the 5000 are the surplus.
    (2) One call brings the rest and the tail: *avail_in is the bytes behind the end, the surplus is empty."""
    from zlibstream_amd import datagen
    plain = datagen.english(4 << 20, 41)
    z = zlib.compress(plain, 6)
    first = 1100000
    assert len(z) > (1 << 20) + 5000 and len(plain) <= ROOM
    tail = random.Random(420).randbytes(4 * first - len(z) + 1000)
    with Stream(engine) as s:
        assert s.call(z[:first], ROOM)[:3] == (ZS_OK, first, b"")
        assert s.call(z[first:] + tail[:5000], ROOM)[:3] == (ZS_OK, len(z) - first + 5000, b"")
        rc, taken, got = s.call(tail[5000:], ROOM)[:3]
        assert (rc, taken) == (ZS_STREAM_END, 0) and got == plain, table(s)
        assert s.surplus() == tail[:5000]
        assert (s.total_in.value, s.total_out.value, s.adler.value) == (len(z), len(plain), zlib.adler32(plain))
    with Stream(engine) as s:
        assert s.call(z[:first], ROOM)[:3] == (ZS_OK, first, b"")
        rc, taken, got = s.call(z[first:] + tail, ROOM)[:3]
        assert (rc, taken) == (ZS_STREAM_END, len(z) - first) and got == plain, table(s)
        assert s.surplus() == b""
        assert (s.total_in.value, s.total_out.value, s.adler.value) == (len(z), len(plain), zlib.adler32(plain))
    print("end found by a call that brings the tail: 2 stream objects")


def test_three_concatenated_streams(engine):
    """Three zlib streams back to back, three stream objects, each started from the surplus of the one before and what the
    caller still held: all three plaintexts come out and nothing is left."""
    cases = [sc.case(n) for n in ("mixed_small", "mixed_probe", "hist_edges_257_one")]
    data = b"".join(c.z for c in cases)
    held = data
    first_call = [len(cases[0].z) + 700, 1500, 1 << 20]  # the first call brings part of the next stream, or all there is
    for c, k in zip(cases, first_call):
        with Stream(engine) as s:
            pos = s.run(held, [(k, ROOM), (0, ROOM), (len(held), ROOM), (0, ROOM)])
            got = b"".join(r[2] for r in s.calls)
            assert got == c.plain and ZS_STREAM_END in [r[0] for r in s.calls], (c.name, table(s))
            assert s.total_in.value == len(c.z) and s.adler.value == zlib.adler32(c.plain)
            assert pos - len(s.surplus()) == len(c.z), (c.name, pos, len(s.surplus()))
            held = s.surplus() + held[pos:]
    assert held == b""
    print("three concatenated streams: 3 stream objects")


# ------------------------------------------------------------------ the buffering threshold
def threshold_child():
    """Run in a process of its own with ZS_INF_PIECE_BYTES=4096: 512 bytes a call, 8 KiB of room, tails behind the streams."""
    from zlibstream_amd import Engine
    engine = Engine(0)
    for name, t in (("tiny_phases", 1), ("ring_wrap", 3000), ("tiny_phases", 700)):
        c = sc.case(name)
        tail = random.Random(430 + t).randbytes(t)
        data = c.z + tail
        with Stream(engine) as s:
            pos, got, pieces = 0, bytearray(), 0
            while True:
                rc, taken, part = s.call(data[pos:pos + 512], 8192)[:3]
                assert rc in (ZS_OK, ZS_STREAM_END), (name, rc, s.message(), table(s))
                # all of a call's bytes or none -- but for the call that meets the end: it leaves what lies behind the trailer
                assert taken in (0, len(data[pos:pos + 512])) or (pos < len(c.z) == pos + taken == s.total_in.value), table(s)
                pieces += 1 if taken and part else 0
                pos += taken
                got += part
                assert s.total_out.value == len(got) and bytes(part) == c.plain[len(got) - len(part):len(got)], (name, table(s))
                if rc == ZS_STREAM_END:
                    break
                assert len(s.calls) < 20000
            assert bytes(got) == c.plain and (s.total_in.value, s.total_out.value) == (len(c.z), len(c.plain)), name
            assert s.adler.value == zlib.adler32(c.plain), name
            assert s.surplus() + data[pos:] == tail, (name, len(s.surplus()), pos, len(data))
            assert pieces >= (1 if name == "tiny_phases" else 20), (name, pieces)  # decoded at calls that brought input: the threshold
            print("%s: %d calls, %d pieces decoded by calls that brought input, surplus %d, left with the caller %d"
                  % (name, len(s.calls), pieces, len(s.surplus()), len(data) - pos))
    print("threshold ok")


def test_buffering_threshold_in_small_calls():
    """zs_inflate's bounded form with the threshold at 4096 bytes (it is read when the library loads: a process of its own):
    tiny_phases and ring_wrap in 512-byte calls with 8 KiB of room, bytes behind their trailers."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_inflate_stream as t; t.threshold_child()" % (os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZS_INF_PIECE_BYTES="4096"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "threshold ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    print(r.stdout.strip())
    print("buffering threshold: 3 stream objects")
