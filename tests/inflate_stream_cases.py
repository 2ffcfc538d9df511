"""zs_inflate taken piece by piece: the catalogue of tests/test_inflate_stream_cases.py (the catalogue's own claims, on the
CPU) and of tests/test_gpu_inflate_stream.py (the device gives exactly the bytes, codes and counters claimed here).  Pure
Python; streams are written block by block with deflate_builder.Builder from fixed seeds, nothing touches the library.

A case is Case(name, z, plain, blocks, schedule, info):
  blocks    the Builder's table with the plaintext length behind every block: (kind, first bit, bits, plaintext end);
            a block of kind "bad" holds a match that reaches before the stream's first byte (too_far) and ends the table;
  schedule  a list of steps (bytes to bring, avail_out); a step with 0 bytes is a call without input;
  info      what a test needs to know of the case's construction (the stated cut, the cuts of a schedule, ...).

The reference.  delivered(case, n) is the plaintext length that the complete blocks in z[:n] hold, which is what calls
without input have handed out in all once n bytes are fed:
  - block k is complete when its last bit is there: (first_bit + bits + 7) // 8 <= n;
  - the final block is complete only with its trailer, n >= len(z).
It is read from zs_inflate_kernel (zlibstream_amd/csrc/zs_inflate.hip): good_bits / good_out are set where a block begins
(line 286: "a block begins here: everything in front of it is complete"), and behind the final block only once all four
trailer bytes are read (lines 460-471: fewer than 32 bits there is "truncated" and leaves both where the final block began);
a stored block whose bytes are not all there (line 299), a code that the input ends in (lines 410-413) or a header cut short
(lines 288, 294, 326, 333) is "truncated" as well, and line 477 turns a piece's "truncated" into ZS_OK at good_bits / good_out.
The host (zs_stream_api.inc, "---- a piece") hands out good_out bytes, drops good_bits >> 3 bytes and resumes at bit
good_bits & 7.  A piece also stops, without an error, in front of a block that does not fit its output buffer when a block
before it did (kInfOutputFull with good_out > pos0): delivered() does not describe the full_output cases, whose test counts
whole blocks instead.  delivered(n) is a prefix of what zlib.decompressobj().decompress(z[:n]) returns, for every n.

expect(case, schedule) is a model of the protocol -- buffer, delivered(), the surplus rule -- and gives per step what the call
returns: (code, bytes taken, bytes given)."""
import collections
import functools
import random
import zlib

import deflate_builder as db
import deflate_reader as dr
import inflate_bad_cases as bc

ZS_OK, ZS_STREAM_END, ZS_DATA_ERROR, ZS_BUF_ERROR = 0, 1, -3, -5
ROOM = 4 << 20  # "room for everything": above every plaintext here
Case = collections.namedtuple("Case", "name z plain blocks schedule info")


class _Builder(db.Builder):
    """Builder that notes the plaintext length behind every block."""

    def __init__(self):
        super().__init__()
        self.ends = []

    def dynamic_block(self, *a, **k):
        r = super().dynamic_block(*a, **k)
        self.ends.append(len(self.plaintext))
        return r

    def stored_block(self, *a, **k):
        r = super().stored_block(*a, **k)
        self.ends.append(len(self.plaintext))
        return r

    def fixed_block(self, *a, **k):
        r = super().fixed_block(*a, **k)
        self.ends.append(len(self.plaintext))
        return r

    def table(self):
        assert len(self.ends) == len(self.blocks)
        return tuple((k, s, n, e) for (k, s, n), e in zip(self.blocks, self.ends))

    def end_byte(self):
        """The first length of the stream that holds every block written so far."""
        return (self.bit_pos + 7) // 8


# ------------------------------------------------------------------ the reference
def block_end_byte(blk):
    return (blk[1] + blk[2] + 7) // 8


def complete_blocks(case, n):
    """How many blocks of the table are complete in z[:n]."""
    k = 0
    for i, blk in enumerate(case.blocks):
        if blk[0] == "bad":
            break
        final = i == len(case.blocks) - 1
        if not (n >= len(case.z) if final else block_end_byte(blk) <= n):
            break
        k = i + 1
    return k


def delivered(case, n):
    k = complete_blocks(case, n)
    return case.blocks[k - 1][3] if k else 0


def resume_phase(case, n):
    """The bit phase 0..7 at which the piece behind a call without input at n bytes begins (None: the stream is through)."""
    k = complete_blocks(case, n)
    return case.blocks[k][1] & 7 if k < len(case.blocks) else None


def block_ends(case):
    """The lengths at which a block becomes complete (the final block: with its trailer)."""
    ends = [block_end_byte(blk) for blk in case.blocks[:-1] if blk[0] != "bad"]
    if case.blocks[-1][0] != "bad":
        ends.append(len(case.z))
    return ends


def cut_schedule(total, cuts, room=ROOM):
    """Feed up to each cut, ask without input; then the rest, and ask again."""
    steps, at = [], 0
    for n in list(cuts) + [total]:
        if n > at:
            steps.append((n - at, room))
        steps.append((0, room))
        at = max(at, n)
    return steps


def expect(case, schedule, tail=b""):
    """The protocol's model for a stream of at most 1 MiB that is never fed past the buffering threshold: per step
    (code, bytes taken, bytes given), and the surplus at the end.  A call that brings input while nothing waits to be read
    is taken in whole and gives nothing; a call without input decodes delivered(fed) and serves it; a call while a piece's
    output waits leaves its input alone and serves.  Bytes behind the trailer (tail) that were fed before the call that met
    the end are the surplus."""
    z, plain = case.z, case.plain
    bad = case.blocks[-1][0] == "bad"
    fed, decoded_to, given, ended, through, surplus, out = 0, 0, 0, False, False, b"", []
    for nbytes, room in schedule:
        if ended:
            out.append((ZS_STREAM_END, 0, b""))
            continue
        taken = 0
        if given == decoded_to and not through:
            if nbytes:
                fed += nbytes
                out.append((ZS_OK, nbytes, b""))
                continue
            if bad and fed >= len(z):
                out.append((ZS_DATA_ERROR, 0, b""))
                continue
            new = delivered(case, fed)
            assert not bad or fed <= block_end_byte(case.blocks[-2]), "a bad block fed in part is not modelled"
            if not bad and fed >= len(z):
                through, surplus = True, (z + tail)[len(z):fed]
            if new == decoded_to and not through:
                out.append((ZS_BUF_ERROR, 0, b""))
                continue
            decoded_to = new
        if room == 0:
            out.append((ZS_BUF_ERROR, taken, b""))
            continue
        k = min(room, decoded_to - given)
        part = plain[given:given + k]
        given += k
        ended = through and given == decoded_to
        out.append((ZS_STREAM_END if ended else ZS_OK, taken, part))
    return out, surplus


# ------------------------------------------------------------------ the streams
def _case(name, b, schedule=None, info=None, z=None, plain=None):
    z = b.finish() if z is None else z
    plain = bytes(b.plaintext) if plain is None else plain
    c = Case(name, z, plain, b.table(), None, dict(info or {}))
    return c._replace(schedule=tuple(schedule) if schedule is not None else tuple(cut_schedule(len(z), block_ends(c)[:-1])))


def _mixed_small():
    """Every block kind, empty blocks of each kind between them, under 1024 bytes: the end is never looked for.  10-bit empty
    fixed blocks are put in until every bit phase has been the first bit of a block."""
    rng = random.Random(301)
    b = _Builder()
    seen = set()

    def lits(n, alphabet=b"abcdefgh"):
        return [rng.choice(alphabet) for _ in range(n)]

    def pad(nonzero=False):
        ph = b.bit_pos & 7
        k = next((k for k in range(4) if (ph + 2 * k) & 7 not in seen and not (nonzero and (ph + 2 * k) & 7 == 0)), 1 if nonzero and ph == 0 else 0)
        for _ in range(k):
            seen.add(b.bit_pos & 7)
            b.fixed_block([], False)
        seen.add(b.bit_pos & 7)

    pad()
    b.dynamic_block(lits(150, b"abcdefghijklmnopqrst ") + [(258, 17), 120, (30, 1)], False)  # a 258-long match, a distance-1 run
    pad()
    b.fixed_block([], False)
    pad(nonzero=True)
    b.stored_block(rng.randbytes(37), False)
    pad()
    b.stored_block(b"", False)  # a flush marker
    pad()
    body = lits(25)
    b.fixed_block(body + [(9, len(b.plaintext) + len(body))], False)  # reaches the stream's first byte
    pad()
    b.dynamic_block(list(rng.randbytes(140)) + [(100, 300)] + lits(11), False)
    pad()
    b.dynamic_block([(258, 1), (258, 1)] + lits(30, b"xyz0123456789") + [(20, 5)], False)
    pad()
    b.dynamic_block(lits(7, b"pq") + [(3, 1)], False)
    pad()
    b.fixed_block([88, 89, (4, 2)], True)
    return _case("mixed_small", b)


def _mixed_probe():
    """inflate_bad_cases.sweep(): 2.4 to 3.1 KB, so that a call without input first runs the finder, the measuring pass and
    the chain on the prefix, and then falls to the piece."""
    z, plain, blocks, _ = bc.sweep()
    rd = dr.read(z)
    ends = [len(dr.replay(rd[:k + 1])) for k in range(len(rd))]
    table = tuple((k, s, n, e) for (k, s, n), e in zip(blocks, ends))
    c = Case("mixed_probe", z, plain, table, None, {})
    return c._replace(schedule=tuple(cut_schedule(len(z), block_ends(c)[:-1])))


HIST_SIZES = (1, 257, 32767, 32768, 32769, 40000)


def _first_part(b, rng, h, many):
    """h bytes of plaintext that end on a block boundary: one block, or blocks of 3 to 5 KiB (a small h: of a third of it; a
    single byte: the byte and a flush marker).  Returns the lengths at which the blocks are complete."""
    cuts, left = [], h
    while left:
        n = left if not many else min(left, rng.randint(3072, 5120) if h > 5120 else max(1, h // 3))
        b.dynamic_block(rng.randbytes(n), False)
        cuts.append(b.end_byte())
        left -= n
    if many and h == 1:
        b.stored_block(b"", False)
        cuts.append(b.end_byte())
    return cuts


def _hist_edges():
    out = []
    for h in HIST_SIZES:
        for many in (False, True):
            rng = random.Random(310 + h)
            b = _Builder()
            cuts = _first_part(b, rng, h, many)
            far = min(h, 32768)
            toks = [(20, far)] + list(rng.randbytes(300)) + [(258, 1)] + list(rng.randbytes(40))  # the first token reaches the oldest byte
            if h + 618 >= 32768:
                toks += [(258, 32768)]
            b.dynamic_block(toks + list(rng.randbytes(5)), False)
            b.fixed_block([69, 78, 68], True)
            z = b.finish()
            out.append(_case("hist_edges_%d_%s" % (h, "many" if many else "one"), b, cut_schedule(len(z), cuts), {"cut": cuts[-1], "cuts": cuts, "h": h}, z=z))
    return out


TOO_FAR_SIZES = (1, 257, 5000)


def _too_far():
    """hist_edges' first match one byte further than there are bytes: cut behind the first part, uncut (the same stream: the
    match sits in the piece that holds the first part), and the legal twin whose match reaches the first byte exactly."""
    out = []
    for h in TOO_FAR_SIZES:
        for legal in (False, True):
            rng = random.Random(330 + h)
            b = _Builder()
            cuts = _first_part(b, rng, h, False)
            if legal:
                b.dynamic_block([(3, h), 66], True)
                out.append(_case("too_far_%d_legal" % h, b, info={"cut": cuts[-1], "h": h}))
                continue
            start = b.bit_pos
            bc._raw_block(b, [(3, h + 1)], True)
            bc._filler(b)
            b.blocks.append(("bad", start, b.bit_pos - start))
            b.ends.append(len(b.plaintext))
            z = b.finish()
            info = {"cut": cuts[-1], "h": h}
            out.append(_case("too_far_%d" % h, b, cut_schedule(len(z), cuts), info, z=z))
            out.append(_case("too_far_%d_uncut" % h, b, cut_schedule(len(z), []), info, z=z))
    return out


RING_PIECE = 200 << 10


def _ring_wrap():
    """A resumed piece of 200 KiB behind 32 768 bytes of history.  The one-wave decoder's ring is 64 KiB and a piece starts at
    ring position 32 768, so piece position p lies at ring position (32768 + p) mod 65536: positions 32767, 65535, 98303, ... are
    the bytes in front of ring positions 0 and 32768.  Matches of length 258 and distance 32 768 are written across the first
    two or three of them, a stored block of 50 000 bytes across the next (_stored: across 98303; ring_wrap: across 131071)."""
    out = []
    for name, matches, stored_at in (("ring_wrap", (32767, 65535, 98303), 131071 - 20000), ("ring_wrap_stored", (32767, 65535), 98303 - 20000)):
        rng = random.Random(340)
        b = _Builder()
        cuts = _first_part(b, rng, 32768, False)
        base = len(b.plaintext)
        toks = []

        def flush():
            if toks:
                b.dynamic_block(toks, False)
                del toks[:]

        def lits_to(p):
            n = p - (len(b.plaintext) - base) - sum(1 if isinstance(t, int) else t[0] for t in toks)
            assert n >= 0
            while n:  # blocks of at most 8000 tokens
                k = min(n, 8000 - len(toks))
                toks.extend(rng.randbytes(k))
                n -= k
                if len(toks) >= 8000:
                    flush()

        for p in matches:
            lits_to(p - 100)
            toks.append((258, 32768))
        lits_to(stored_at)
        flush()
        b.stored_block(rng.randbytes(50000), False)
        lits_to(RING_PIECE)
        flush()
        assert len(b.plaintext) - base == RING_PIECE
        b.fixed_block([69, 78, 68], True)
        z = b.finish()
        info = {"cut": cuts[-1], "matches": matches, "stored": (stored_at, stored_at + 50000)}
        out.append(_case(name, b, cut_schedule(len(z), cuts), info, z=z))
    return out


def _full_output():
    """Blocks of about 600 KiB of plaintext in a few hundred bytes each: a piece's first output buffer is max(8 x in_len, 1 MiB),
    so a piece takes one block and stops in front of the next.  The last byte of the trailer is held back, or the end would be
    found and the whole stream decoded at once.  The twin is one block of exactly 3 MiB: nothing fits, the buffer grows."""
    b = _Builder()
    for k in range(6):
        b.dynamic_block([65 + k] + [(258, 1)] * 2381, False)
    b.fixed_block([69, 78, 68], True)
    z = b.finish()
    steps = [(len(z) - 1, ROOM)] + [(0, ROOM)] * 7 + [(1, ROOM), (0, ROOM)]
    out = [_case("full_output", b, steps, z=z)]
    b = _Builder()
    b.dynamic_block([90] + [(258, 1)] * 12192 + [(191, 1)], False)
    assert len(b.plaintext) == 3 << 20
    b.fixed_block([], True)
    z = b.finish()
    out.append(_case("full_output_twin", b, [(len(z) - 1, ROOM), (0, ROOM), (1, ROOM), (0, ROOM)], z=z))
    return out


def _tiny_phases():
    """300 blocks of 1 to 40 literals, fixed and dynamic, with 0 to 3 empty fixed blocks (10 bits) in front of each; the
    schedule cuts behind every one of the 300."""
    rng = random.Random(350)
    b = _Builder()
    cuts = []
    for i in range(300):
        for _ in range(rng.randrange(4)):
            b.fixed_block([], False)
        toks = [rng.choice(b"etaoin shrdlu") for _ in range(rng.randint(1, 40))]
        if rng.random() < 0.5:
            b.fixed_block(toks, False)
        else:
            b.dynamic_block(toks, False)
        cuts.append(b.end_byte())
    b.fixed_block([], True)
    z = b.finish()
    return _case("tiny_phases", b, cut_schedule(len(z), cuts), {"cuts": cuts}, z=z)


@functools.lru_cache(maxsize=None)
def catalogue():
    cases = [_mixed_small(), _mixed_probe()] + _hist_edges() + _too_far() + _ring_wrap() + _full_output() + [_tiny_phases()]
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def case_names():
    """The catalogue's names without building it (for parametrised tests)."""
    return (["mixed_small", "mixed_probe"] + ["hist_edges_%d_%s" % (h, f) for h in HIST_SIZES for f in ("one", "many")] +
            ["too_far_%d%s" % (h, s) for h in TOO_FAR_SIZES for s in ("", "_uncut", "_legal")] +
            ["ring_wrap", "ring_wrap_stored", "full_output", "full_output_twin", "tiny_phases"])


def case(name):
    return next(c for c in catalogue() if c.name == name)


def is_bad(c):
    return c.blocks[-1][0] == "bad"
