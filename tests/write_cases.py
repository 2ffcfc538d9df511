"""Write schedules at the edges of Fill_window's read rules -- when the reference reads, slides the window and inserts a position
ahead of its turn -- which the regular Write sizes of tests/test_gpu_parity.py and the fuzzers meet only by chance.

A case is (name, data, level, strategy, ends, flushes, claim, route).  `ends` are the cumulative Write ends, the last one the
stream's length; `flushes` is None (every Write under NoFlush) or a flush mode per Write (the resume family: the first alone).  The claim is a predicate over the ORACLE's trace of that schedule
-- claim(tokens, reads, slides): match_cases.tokens of its stream, and Oracle.trace's read events (loop-top, bytes read,
pre-insert ran, window base) and slide events (loop-top, new base) -- and says which side of its rule's edge the case is on.  The
sides of an edge are twins: the same bytes, Write lists that differ by the one byte or the one Write the rule turns on (the few
edges that turn on the data instead -- eq_bucket, nil -- say so).  tests/test_write_cases.py holds every claim against the oracle,
holds it false on the twin's trace, and runs every case through the CPU model and the host's verdicts
(tests/cpp/test_write_verdicts.cpp); tests/test_gpu_write_cases.py asks the device for the oracle's bytes.  A claim is never
evaluated on the device's stream.

`route` is what the planner must do with the case: "bulk" (levels 4-9: the chunked form up to n - 262), "bulk_tail" (the body
ends early, the tail engine takes the last cluster), "literal" (the one-wave literal engine, whole), "poisoned" (bulk first; the
resolve kernel flags the stream and the batch runs again with it on the literal engine), "sweeps" (levels 1-3), "folded" (Rle: run
as one Write), "resumed" (the run behind a flushed Write goes on in the parallel forms from the flush; "literal" there: that run
stays with the literal engine).  ROUTE_ONLY names the cases that have no claim about the stream: the rule they pin says who runs the stream, not
what it says.

How an event shows in the tokens.  Fill_window inserts loop-top + 1 after every read (oracle/zs_oracle.c fill_window; Deflate.cs
:1010-1013), so when the parse reaches that position its bucket's head is the position itself and its search does not happen.
A *probe* is a planted match of 12 bytes at position q: found at q in one Write; with an event at q - 1 the stream has a literal
at q and the match's last 11 bytes at q + 1; with an event at q as well, two literals and 10 bytes.  At levels 1-3 a position
inside a match longer than max_insert is never inserted unless an event does it: there a later copy of the bytes from q on finds
q (long) or the match's source (short).

What an event cannot show.  An event whose loop-top + 1 is a literal's position, or lies inside a match that is emitted anyway,
leaves the single Write's tokens: of two Write ends one byte apart at most one kills a search (levels 4-9).  Such a side of an
edge carries an *anchor*: one more Write end at _A0 = 20000, the same on both sides, whose event kills a probe of its own, so
that no case's stream is the single Write's; the edge itself then shows in how the twins differ -- in the probe's tokens where
the rule moves a pre-insert, in the oracle's read and slide events alone where it moves only which loop-top reads (slide_early,
poison: the docstrings say so).

Families, with what each guards (zlibstream_amd/csrc/zs_core.h unless named):
  event_top     chunk_special_prefix's event test `p >= B - (kMinLookahead - 1)`, eq_here / pre_eq and the three was_pre branches;
                zs_fast_sweep.h's events
  lookahead     chunk_special_prefix's read loop `E - p >= kMinLookahead`; build_read_events' `r < kMinLookahead`
  cluster       build_geometry: kClusterGap (270 = 262 + 8), kClusterSpanMax (1500), kClusterMax (64)
  slide         chunk_special_prefix: `p >= cx.S`, the window-bit skip `ei++` when slid, nil_edge; build_geometry: window_tail,
                seg_S / seg_base of a second window, a Write end on a window end (kClWindowBit clear)
  tail_handover build_geometry's exits: the dropped last cluster (2 * kMinLookahead = 524 from the end), the stale bytes behind
                an early slide, a first cluster with nothing in front of it
  poison        chunk_special_prefix's `E - p < 7` (kMapPoisonBit)
  fast_events   build_read_events(any_end = true): `r < kMinLookahead`, `lo < kSlideAt` / `hi >= kSlideAt`, the read capped by the
                window's room; fs_event_nil_edge (zs_fast_sweep.h)
  rle_fold      fold_rle_writes (zs_plan.h): `E >= kWindowSize - kMinLookahead && E % kWSize >= kWSize - kMinLookahead`
  resume        GeoStart (build_geometry) and build_read_events' E_start: a first Write under a Sync or Full flush, NoFlush Writes
                behind it -- a flush at 65273 / 65274 (the flush itself slides a window that stands on the threshold), a run of
                524 / 523 bytes behind the flush (`body_end < p0 + kMinLookahead`; zs_plan.h `len - p0 >= 2 * kMinLookahead`), and
                the Write lists of the cluster, lookahead and fast_events families behind a flush.  GeoStart's exits that no
                stream reaches (`p0 >= kSlideAt` at a read, `E0 - p0 < kMinLookahead` in the middle of a Write) are rows of
                tests/test_write_cases.py's test_geostart_verdicts.

rle_fold is route-only.  What a Write end could move under Rle is the loop-top at which the window slides, and with it a
block's permission to be stored (block_start >= 0 after the slide), so the input to look for is one whose block is open across
the slide, began more than 32 506 bytes in front of it, and is smaller stored than coded.  A block holds 16 383 symbols.  Of
incompressible bytes that is 16 383 literals: the blocks end at multiples of 16 383, the fourth at 65 532 -- inside 65 274 ..
65 536 by nature, no alignment needed -- and begin 16 383 bytes in front: the permission never moves.  A block that spans 32 506
bytes is at least half runs, which Rle codes far below their stored size: it is never stored.  Between the two, tried on the
CPU at levels 1 and 6 with a Write end at every position of 65 274 .. 65 536 and every third of 98 042 .. 98 304: random bytes;
66 000 random bytes then zeros; random bytes then two-valued bytes from 65 200 + 16 k on (k = 2, 6, 10: the last literal block's
end moved across the slide); random bytes each repeated 1, 1, 1, 2 or 3 times (blocks of more bytes than symbols).  No stream changed.

Seeds were tuned on the CPU until the claims held (_SEEDS), and are frozen."""
import functools

import match_cases as mc
from match_cases import DEFAULT, RLE, MAX_DIST

HIGH = bytes(range(0x80, 0x100))
W1, W2, WS = 65536, 98304, 32768
LA = 262          # kMinLookahead
SLIDE_AT = 65274  # kSlideAt


# ------------------------------------------------------------------ the oracle's events
def after(reads, E):
    """loop-top of the read that follows data end E (the first read of the Write behind E, or of the window's next part)"""
    at = 0
    for top, n, pre, base in reads:
        if at == E:
            return top
        at += n
    return None


def reads_at(reads, top):
    return [r for r in reads if r[0] == top]


def tops(reads):
    out = []
    for r in reads:
        if not out or out[-1] != r[0]:
            out.append(r[0])
    return out


def _hits(t, kills):
    """kills: {probe (position q, distance d): k}.  A probe is a planted match of 12 bytes; k searches killed from q on (an event
    at q - 1 kills the search at q; an event at q as well kills the one at q + 1) leave k literals and the match's last 12 - k."""
    for (q, d), k in kills.items():
        if any(t.get(q + j) != (1, 0) for j in range(k)) or t.get(q + k) != (12 - k, d):
            return False
    return True


def boundaries(n, ends):
    """the data ends of a schedule, restated from the rule: 0, the Write ends and the window ends below n, in order"""
    b, x, last, w = [0], W1, 0, 0
    while True:
        while w < len(ends) and ends[w] <= last:
            w += 1
        we = ends[w] if w < len(ends) else n
        nx = min(we, x)
        if nx >= n:
            break
        b.append(nx)
        last = nx
        if nx == x:
            x += WS
    return b


def read_ends(n, ends):
    """The data ends one after the other as Fill_window's reads make them, restated from the rule for schedules whose reads all
    bring a full lookahead: a read takes the rest of its Write or the window's room, and the window slides in front of it when
    the data read so far reaches 65274 bytes into the window or further."""
    E, base, w, out = 0, 0, 0, []
    while E < n:
        if E - base >= SLIDE_AT:
            base += WS
        while ends[w] <= E:
            w += 1
        E += min(W1 - (E - base), ends[w] - E)
        out.append(E)
    return out


def expected_segments(n, ends):
    """Boundaries per segment as build_geometry must cluster them: boundaries (a Write end on a window end is a Write end) at most
    270 apart are one cluster; the first read alone is a segment without a cluster."""
    b = boundaries(n, ends)
    out, i = [], 0
    while i < len(b):
        j = i + 1
        while j < len(b) and b[j] - b[j - 1] <= 270:
            j += 1
        out.append(0 if i == 0 and j == 1 else j - i)
        i = j
    return out


# ------------------------------------------------------------------ building blocks
class _Layout:
    """Strings at fixed positions, filler (match_cases._B) between them."""

    def __init__(self, seed, n):
        self.b = mc._B(seed)
        self.rng = self.b.rng
        self.n = n
        self.segs = []
        self.g = 0

    def guard(self):
        self.g += 1
        return bytes([0x20 + self.g % 32])

    def high(self, k):
        return bytes(self.rng.choices(HIGH, k=k))

    def at(self, pos, bs):
        self.segs.append((pos, bytes(bs)))

    def pair(self, src, tgt, X, front=True):
        """X at src and at tgt, each between bytes that end the repeat on both sides (front=False: the byte in front of the target
        is another string's closing byte); returns the target's closing byte"""
        self.at(src - 1, self.guard() + X + self.guard())
        closing = self.guard()
        if front:
            self.at(tgt - 1, self.guard() + X + closing)
        else:
            self.at(tgt, X + closing)
        return closing

    def probe(self, q, z, front=True):
        """a planted match of 12 bytes at q whose source is at z: (q, distance)"""
        self.pair(z, q, self.b.rand(12), front)
        return q, q - z

    def bytes(self):
        b = self.b
        for pos, bs in sorted(self.segs):
            assert pos >= len(b), ("segments overlap", pos, len(b))
            b.fill_to(pos)
            b.put(bs)
        b.fill_to(self.n)
        return b.bytes()


_SPECS = []
META = {}
ROUTE_ONLY = set()


def _add(family, edge, side, name, level, build, ends, route, strategy=DEFAULT, route_only=False, flushes=None):
    assert name not in META, name
    META[name] = (family, edge, side)
    if route_only:
        ROUTE_ONLY.add(name)
    assert flushes is None or len(flushes) == len(ends)
    _SPECS.append((name, level, strategy, tuple(ends), route, build, flushes))


def _fast(level):
    return level <= 3


_B0, _N0, _A0 = 40000, 67000, 20000


def _anchor(L):
    """The probe of the anchor Write end _A0 (see the module's docstring): its event stands at _A0 - 261."""
    return L.probe(_A0 - 260, _A0 - 3000)


# ------------------------------------------------------------------ event_top
def _event_top_data(level):
    """A 20-byte match M at T whose loop-tops are B - 262 (levels 4-9: B - 263 and B - 262) and then its closing byte.  A Write
    that ends at B fires at the closing byte and kills the probe behind it; one that ends at B - 1 fires at B - 262 and inserts
    B - 261, inside M, ahead: nothing at levels 4-9 (the anchor keeps the stream off the single Write's); at levels 1-3, where the
    inside of a match longer than max_insert is not inserted, a later copy of the bytes from B - 261 on finds them there."""
    fast = _fast(level)
    T = _B0 - 262 if fast else _B0 - 263

    def build(seed):
        L = _Layout(seed, _N0)
        X, S = L.b.rand(20), T - 6000
        e_out, e_in = T + 20, _B0 - 262
        closing = L.pair(S, T, X)
        pr = L.probe(e_out + 1, T - 800, front=False)
        an = _anchor(L)
        yp = _B0 + 700
        data = L.bytes()
        if fast:  # 19 bytes of M, its closing byte, two of the probe
            data = data[:yp - 1] + b"\x3f" + data[T + 1:T + 23] + b"\x3e" + data[yp + 23:]
        assert closing[0] == data[e_out]

        def claim_out(t, reads, slides):
            ok = after(reads, _B0) == e_out and t.get(T) == (20, 6000) and _hits(t, {pr: 1, an: 1})
            return ok and (not fast or t.get(yp) == (19, yp - (S + 1)))

        def claim_in(t, reads, slides):
            ok = after(reads, _B0 - 1) == e_in and t.get(T) == (20, 6000) and _hits(t, {pr: 0, an: 1})
            return ok and (not fast or t.get(yp) == (22, yp - (T + 1)))
        return data, {"out": claim_out, "in": claim_in}
    return build


def _adjacent_data(level):
    """Literals and a probe at B - 260.  Write ends at B and B + 1 fire at B - 261 and B - 260 -- the second event at the position
    the first one inserted ahead, reached over a literal: the probe is found two positions late.  Write ends at B and B + 2 fire
    at B - 261 and B - 259: one position late."""
    def build(seed):
        L = _Layout(seed, _N0)
        L.at(_B0 - 270, L.high(9))
        pr = L.probe(_B0 - 260, _B0 - 1500)
        data = L.bytes()

        def claim(second, kills):
            def c(t, reads, slides):
                return after(reads, _B0) == _B0 - 261 and after(reads, _B0 + second) == _B0 - 261 + second and _hits(t, {pr: kills})
            return c
        return data, {"in": claim(1, 2), "out": claim(2, 1)}
    return build


def _eq_data(level, period, where):
    """A run of one period across an event loop-top e.  Period 1: e and e + 1 share their bucket -- the search at e is dead, the
    one at e + 1 sees e alone (a distance-1 match through run1).  Period 2: they do not.  where: "mid" (a Write ends inside the
    run), "pair" (two Write ends one byte apart), "start" (the stream begins with the run and a Write ends 100 bytes in: the
    event at loop-top 0 inserts position 1, whose only candidate is position 0, "none": `p > 1`).  These sides turn on the data,
    not on the Write list."""
    def build(seed):
        L = _Layout(seed, _N0)
        unit = bytes(L.rng.sample(list(mc.ALPHA), period))
        at = 0 if where == "start" else _B0 - 700
        if where == "start":
            L.at(0, (unit * 600)[:600] + L.guard())
        else:
            L.at(at - 1, L.guard() + (unit * 900)[:900] + L.guard())
        an = _anchor(L)
        data = L.bytes()
        first = 100 if where == "start" else _B0

        def claim(t, reads, slides, hv=0):
            e = after(reads, first)
            if e is None or not at <= e < at + 590 or not _hits(t, {an: 1}):
                return False
            same = mc._buckets(data, hv)[e] == mc._buckets(data, hv)[e + 1]
            return same == (period == 1) and (where != "pair" or after(reads, first + 1) is not None)
        return data, {"in": claim, "out": claim}
    return build


def _event_top_cases():
    for level in (1, 3, 4, 6, 9):
        d = _event_top_data(level)
        for side, end in (("out", _B0), ("in", _B0 - 1)):
            _add("event_top", "b261_L%d" % level, side, "top_%s_L%d" % ("behind_match" if side == "out" else "on_b261", level), level, (d, side), [_A0, end, _N0],
                 "sweeps" if _fast(level) else "bulk")
    for level in (1, 6, 9):
        d = _adjacent_data(level)
        for side, second in (("in", 1), ("out", 2)):
            _add("event_top", "adjacent_L%d" % level, side, "adjacent_plus%d_L%d" % (second, level), level, (d, side), [_B0, _B0 + second, _N0],
                 "literal" if _fast(level) else "bulk")
    for level in (6, 1, 4, 9):
        for where, ends in (("mid", [_A0, _B0, _N0]), ("pair", [_A0, _B0, _B0 + 1, _N0]), ("start", [100, _A0, _N0])):
            if level in (4, 9) and where != "mid":
                continue
            for period in (1, 2):
                fast_route = "literal" if where != "mid" else "sweeps"
                _add("event_top", "eq_bucket_%s_L%d" % (where, level), "in" if period == 1 else "out", "eq_%s_p%d_L%d" % (where, period, level), level,
                     (_eq_data(level, period, where), "in"), ends, fast_route if _fast(level) else "bulk")


# ------------------------------------------------------------------ lookahead
def _lookahead_data(level):
    """A 250-byte match M so that the event of a Write end B stands at e = B - 12 (levels 1-3) or B - 13 with that many bytes
    ahead: how many Writes the one loop-top reads is then a question of their sizes.  A probe at e + 1."""
    fast = _fast(level)
    T = _B0 - 262 if fast else _B0 - 263
    e = T + 250  # M's closing byte
    la = _B0 - e

    def build(seed):
        L = _Layout(seed, _N0)
        L.pair(T - 9000, T, L.b.rand(250))
        pr = L.probe(e + 1, T - 1200, front=False)
        data = L.bytes()
        return data, {
            # the Write behind B brings the lookahead to 261: the loop-top reads once more ...
            ("w261", "in"): lambda t, r, s: len(reads_at(r, e)) == 2 and after(r, _B0 + 261 - la) == e and _hits(t, {pr: 1}),
            # ... to 262: it does not, and the next loop-top is an event
            ("w261", "out"): lambda t, r, s: len(reads_at(r, e)) == 1 and after(r, _B0 + 262 - la) == e + 1 and _hits(t, {pr: 2}),
            # Writes of 1, 3, 100 and 261 bytes behind B: all four are read at e ...
            ("chain", "in"): lambda t, r, s: len(reads_at(r, e)) == 4 and not reads_at(r, e + 1) and _hits(t, {pr: 1}),
            # ... the third one longer, so that it brings the lookahead to 262: the fourth is read at e + 1
            ("chain", "out"): lambda t, r, s: len(reads_at(r, e)) == 3 and len(reads_at(r, e + 1)) == 1 and _hits(t, {pr: 2})}
    return build, la


def _lookahead_cases():
    for level in (1, 6, 9):
        fast = _fast(level)
        d, la = _lookahead_data(level)
        for side, w in (("in", 261 - la), ("out", 262 - la)):
            _add("lookahead", "w261_L%d" % level, side, "ahead_%d_L%d" % (la + w, level), level, (d, ("w261", side)), [_B0, _B0 + w, _N0], "literal" if fast else "bulk")
        for side, third in (("in", 100), ("out", 262 - la - 4)):
            _add("lookahead", "chain_L%d" % level, side, "chain_%s_L%d" % ("one_top" if side == "in" else "two_tops", level), level, (d, ("chain", side)),
                 [_B0, _B0 + 1, _B0 + 4, _B0 + 4 + third, _B0 + 4 + third + 261, _N0], "literal" if fast else "bulk")


# ------------------------------------------------------------------ cluster
def _cluster_data(level, gap_in):
    """Write ends at B and B + gap, a probe behind each event: B - 260, and B + gap_in - 260 (killed on the `in` side; on the
    other the second event stands on the probe itself)."""
    def build(seed):
        L = _Layout(seed, _N0)
        p1, p2 = L.probe(_B0 - 260, _B0 - 1500), L.probe(_B0 + gap_in - 260, _B0 - 1400)
        data = L.bytes()

        def claim(gap):
            def c(t, reads, slides):
                return after(reads, _B0) == _B0 - 261 and after(reads, _B0 + gap) == _B0 + gap - 261 and _hits(t, {p1: 1, p2: 1 if gap == gap_in else 0})
            return c
        return data, {gap: claim(gap) for gap in (gap_in, gap_in + 1)}
    return build


def _plain_data(n):
    def build(seed):
        return _Layout(seed, n).bytes(), {None: None}
    return build


def _cluster_cases():
    for level in (6, 4):
        for gap_in in (262, 270):
            d = _cluster_data(level, gap_in)
            for gap in (gap_in, gap_in + 1):
                _add("cluster", "gap%d_L%d" % (gap_in, level), "in" if gap == gap_in else "out", "gap_%d_L%d" % (gap, level), level, (d, gap), [_B0, _B0 + gap, _N0], "bulk")
    d = _plain_data(_N0)
    # seven Write ends 250 apart: first to last 1500; six and one at + 1501
    _add("cluster", "span", "in", "span_1500", 6, (d, None), [_B0 + 250 * i for i in range(7)] + [_N0], "bulk", route_only=True)
    _add("cluster", "span", "out", "span_1501", 6, (d, None), [_B0 + 250 * i for i in range(6)] + [_B0 + 1501, _N0], "literal", route_only=True)
    # 64 boundaries 20 apart are one cluster; 65 are one too many
    _add("cluster", "count", "in", "count_64", 6, (d, None), [_B0 + 20 * i for i in range(64)] + [_N0], "bulk", route_only=True)
    _add("cluster", "count", "out", "count_65", 6, (d, None), [_B0 + 20 * i for i in range(65)] + [_N0], "literal", route_only=True)


# ------------------------------------------------------------------ slide
_SLIDE_PAIRS = ((-263, -262), (-2, -1), (0, 1))   # Write ends against a window end W: 65273 / 65274, 65534 / 65535, 65536 / 65537


def _len_for(W):
    return 100000 if W == W1 else 133000


def _slide_data(level, W, pair, n=None):
    """Literals around the events of the Write ends W + pair[0] and W + pair[1], a probe behind the later one's: a Write end in
    the last 262 bytes of the window or not (65273 / 65274); its event below the slide threshold or on it (65534 / 65535: the
    window slides at 65274, not at 65275); a Write that ends with the window or a byte behind it (65536 / 65537: the window end's
    event reads one byte, the next loop-top is an event again).  The anchor keeps the sides that are the single Write's stream
    by nature off it: 65273 and 65534 (the position inserted ahead is a literal's) and 65536 (the single Write's own read)."""
    def build(seed):
        L = _Layout(seed, n or _len_for(W))
        e_late = W + pair[1] - 261
        L.at(e_late - 12, L.high(12))
        pr = L.probe(e_late + 1, W - 2600)
        an = _anchor(L)
        data = L.bytes()
        base = W - W1  # the window's base in front of this window end

        def claim(off):
            E = W + off
            e = E - 261

            def c(t, reads, slides):
                if after(reads, E) != e:
                    return False
                sl = [s for s in slides if s[1] == base + WS]
                # the window slides at the first event at or behind base + 65274: the Write end's own, or the window end's (W - 261)
                slide_at = e if base + SLIDE_AT <= e <= W - 261 else W - 261
                return len(sl) == 1 and sl[0][0] == slide_at and _hits(t, {pr: 1 if off == pair[1] else 0, an: 1})
            return c
        return data, {off: claim(off) for off in pair}
    return build


def _early_data(level, W):
    """A 258-byte match whose loop-tops are W - 398 (levels 4-9: W - 399 and W - 398) and then its closing byte, behind the slide
    threshold.  A Write that ends at W - 136 fires there and slides the window early -- the window's end is then no limit to its
    read, the cluster's window bit is skipped; one that ends at W - 137 fires at W - 398, and the window end's own event slides.
    The stream is the same either way, and the single Write's but for the anchor: the sides differ in their events alone."""
    fast = _fast(level)
    T = W - 398 if fast else W - 399
    e2 = T + 258

    def build(seed):
        L = _Layout(seed, _len_for(W))
        L.pair(T - 7000, T, L.b.rand(258))
        pr = L.probe(e2 + 1, T - 1000, front=False)
        an = _anchor(L)
        data = L.bytes()
        base = W - W1

        def claim(early):
            def c(t, reads, slides):
                sl = [s for s in slides if s[1] == base + WS]
                if len(sl) != 1 or sl[0][0] != e2 or not _hits(t, {pr: 1, an: 1}) or t.get(T) != (258, 7000):
                    return False
                E = W - 136 if early else W - 137
                return after(reads, E) == (e2 if early else W - 398) and len([x for x in tops(reads) if W - 400 <= x <= e2]) == (1 if early else 2)
            return c
        return data, {"in": claim(True), "out": claim(False)}
    return build


def _nil_data(level, W, dist):
    """match_cases' slide at a Write end, on both sides of the distance: a repeat planted at T = W - 262 whose source lies `dist`
    back.  A Write that ends at W - 1 fires at T = the slide threshold, the window slides there, and a source at distance 32506
    is window index 0 now, "none": the match begins two positions later.  At 32505 it is found.  (The sides turn on the data.)"""
    T = W - 262

    def build(seed):
        L = _Layout(seed, _len_for(W))
        L.pair(T - dist, T, L.b.rand(100))
        an = _anchor(L)
        data = L.bytes()

        def claim(t, reads, slides, hv=0):
            if mc.mates(data, T, T - dist, hv) != [T - dist] or after(reads, W - 1) != T or (T, W - W1 + WS) not in slides or not _hits(t, {an: 1}):
                return False
            if dist < MAX_DIST:
                return t.get(T) == (100, dist)
            return t.get(T) == (1, 0) and t.get(T + 1) == (1, 0) and t.get(T + 2) == (98, dist)
        return data, {"in": claim, "out": claim}
    return build


def _slide_cases():
    for level in (6, 1):
        for W in (W1, W2):
            for pair, edge in zip(_SLIDE_PAIRS, ("tail_lo", "tail_hi", "window_end")):
                d = _slide_data(level, W, pair)
                for off in pair:
                    E = W + off
                    fast_route = "literal" if -262 <= off <= -2 or off == 1 else "sweeps"  # (65537: the window end's read brings one byte)
                    _add("slide", "%s_%d_L%d" % (edge, W, level), "in" if off in (-262, -1, 0) else "out", "slide_end_%d_L%d" % (E, level), level, (d, off),
                         [_A0, E, _len_for(W)], fast_route if _fast(level) else "bulk")
            d = _early_data(level, W)
            for side, E in (("in", W - 136), ("out", W - 137)):
                _add("slide", "early_%d_L%d" % (W, level), side, "slide_early_end_%d_L%d" % (E, level), level, (d, side), [_A0, E, _len_for(W)],
                     "literal" if _fast(level) else "bulk")
            for dist, side in ((MAX_DIST, "in"), (MAX_DIST - 1, "out")):
                _add("slide", "nil_%d_L%d" % (W, level), side, "slide_nil_%d_dist%d_L%d" % (W, dist, level), level, (_nil_data(level, W, dist), side),
                     [_A0, W - 1, _len_for(W)], "sweeps" if _fast(level) else "bulk")


# ------------------------------------------------------------------ tail_handover
def _tail_data(n, probes):
    """literals and a probe behind the events of the boundaries of `probes`; the claim is for one schedule's Write ends"""
    def build(seed):
        L = _Layout(seed, n)
        pr = {}
        for i, B in enumerate(probes):
            L.at(B - 272, L.high(11))
            pr[B] = L.probe(B - 260, B - 3000 - 40 * i)
        data = L.bytes()

        def claim(ends):
            def c(t, reads, slides):
                return all(after(reads, B) == B - 261 for B in ends) and _hits(t, {pr[B]: 1 if B in ends else 0 for B in pr})
            return c
        return data, claim
    return build


def _tail_cases():
    for level in (6, 9):
        n = 70000
        # a last cluster of two boundaries whose second lies within 524 bytes of the end is the tail engine's; a lone boundary is not
        d = _tail_data(n, (n - 500, n - 300))
        _add("tail_handover", "drop_L%d" % level, "in", "tail_two_ends_L%d" % level, level, (d, (n - 500, n - 300)), [n - 500, n - 300, n], "bulk_tail")
        _add("tail_handover", "drop_L%d" % level, "out", "tail_one_end_L%d" % level, level, (d, (n - 300,)), [n - 300, n], "bulk")
        d = _tail_data(n, (n - 700, n - 523))
        _add("tail_handover", "edge524_L%d" % level, "out", "tail_last_at_524_L%d" % level, level, (d, (n - 700,)), [n - 700, n - 524, n], "bulk")
        _add("tail_handover", "edge524_L%d" % level, "in", "tail_last_at_523_L%d" % level, level, (d, (n - 700, n - 523)), [n - 700, n - 523, n], "bulk_tail")
        # a Write end in the last 262 bytes of a window (it slides early) and a stream that ends where the window's stale bytes would
        # be read: n % 32768 >= 32768 - 524.  (Twins by the stream's last byte.)
        for m, side, route in ((W2 - 524 - 1, "out", "bulk"), (W2 - 524, "in", "literal")):
            d = _tail_data(m, (W1 - 1,))
            _add("tail_handover", "stale_L%d" % level, side, "tail_stale_n%d_L%d" % (m, level), level, (d, (W1 - 1,)), [W1 - 1, m], route)
    # window_tail's two comparisons, where they decide: a Write end at window index 65274 / 65273 of a stream that ends with the
    # window (no window end behind it in the stream: the tail engine's), and of streams that end in the stale bytes, in the first
    # window (both comparisons turn at 65274) and in the second (the first one is long true)
    for W, n, tag, route in ((W1, W1, "short", "bulk_tail"), (W1, W2 - 524, "stale_lo", "literal"), (W2, W2 + WS - 524, "stale_w2", "literal")):
        d = _slide_data(6, W, _SLIDE_PAIRS[0], n)
        for off in _SLIDE_PAIRS[0]:
            _add("tail_handover", "window_tail_%s" % tag, "in" if off == -262 else "out", "tail_%s_end_%d" % (tag, W + off), 6, (d, off), [_A0, W + off, n],
                 route if off == -262 else "bulk")
    # A first cluster (the stream's start and a Write end 200 bytes in) with nothing in front of its last boundary + 524.
    # Route-only, and it cannot be otherwise: the lookahead at loop-top 0 is 200, so the second Write is read there too -- the
    # Write end's event is the stream's first loop-top, whose pre-insert of position 1 the single Write does as well (and
    # position 1 has no candidate but position 0, "none"): the stream is the single Write's whatever the bytes are.
    for n, side, route in ((723, "in", "literal"), (724, "out", "bulk")):
        d = _plain_data(n)
        _add("tail_handover", "first_cluster", side, "tail_first_cluster_n%d" % n, 6, (d, None), [200, n], route, route_only=True)
    # the lengths: one Write of 261 bytes has no loop-top with a full lookahead (build_geometry's `n < kMinLookahead`, the
    # planner's `len >= kMinLookahead`); one of 262 has one, loop-top 0, and at levels 1-3 the sweeps take it.  (Levels 4-9 leave
    # both to the literal engine: their body wants 262 loop-tops, n = 524.)
    for level in (1, 3):
        for n, side, route in ((261, "out", "literal"), (262, "in", "sweeps")):
            _add("tail_handover", "length_L%d" % level, side, "tail_length_%d_L%d" % (n, level), level, (_plain_data(n), None), [n], route, route_only=True)


# ------------------------------------------------------------------ poison
def _poison_data(level):
    """A 258-byte match so that the event of a Write end B stands at B - 5 with five bytes ahead: a Write of one byte behind B
    leaves six, and the pre-insert of B - 4 hashes the bytes B - 2 .. B + 1: one behind the data.  A Write of two leaves seven.
    The stream is the same either way (the probe at B - 4 is killed): the sides differ in their events alone."""
    T = _B0 - 263
    e = T + 258

    def build(seed):
        L = _Layout(seed, _N0)
        L.pair(T - 9000, T, L.b.rand(258))
        pr = L.probe(e + 1, T - 1000, front=False)
        data = L.bytes()

        def short(reads):
            at, out = 0, []
            for top, n, pre, base in reads:
                at += n
                if pre and at - top < 7 and top > 0:
                    out.append(top)
            return out

        def claim(poisoned):
            def c(t, reads, slides):
                return after(reads, _B0) == e and short(reads) == ([e] if poisoned else []) and t.get(T) == (258, 9000) and _hits(t, {pr: 1})
            return c
        return data, {"in": claim(True), "out": claim(False)}
    return build


def _poison_cases():
    for level in (6, 9):
        d = _poison_data(level)
        _add("poison", "e_minus_p_L%d" % level, "in", "poison_six_ahead_L%d" % level, level, (d, "in"), [_B0, _B0 + 1, _N0], "poisoned")
        _add("poison", "e_minus_p_L%d" % level, "out", "poison_seven_ahead_L%d" % level, level, (d, "out"), [_B0, _B0 + 2, _N0], "bulk")
        _add("poison", "short_writes_L%d" % level, "in", "poison_writes_1_2_3_L%d" % level, level, (d, "in"), [_B0, _B0 + 1, _B0 + 3, _B0 + 6, _N0], "poisoned")
        _add("poison", "short_writes_L%d" % level, "out", "poison_writes_2_1_3_L%d" % level, level, (d, "out"), [_B0, _B0 + 2, _B0 + 3, _B0 + 6, _N0], "bulk")


# ------------------------------------------------------------------ fast_events
def _fast_read_data(level):
    """Write ends at B and B + 261 / B + 262: the read at B - 261 brings 261 bytes (the lookahead is 522: enough, but the sweeps
    want every read to bring a full lookahead) or 262.  Probes behind both events."""
    def build(seed):
        L = _Layout(seed, _N0)
        p1, p2 = L.probe(_B0 - 260, _B0 - 1500), L.probe(_B0 + 1, _B0 - 1400)
        data = L.bytes()

        def claim(w):
            def c(t, reads, slides):
                r = reads_at(reads, _B0 - 261)
                return len(r) == 1 and r[0][1] == w and after(reads, _B0 + w) == _B0 + w - 261 and _hits(t, {p1: 1, p2: 1 if w == 261 else 0})
            return c
        return data, {w: claim(w) for w in (261, 262)}
    return build


def _fast_cases():
    for level in (1, 2, 3):
        d = _fast_read_data(level)
        _add("fast_events", "read261_L%d" % level, "in", "fast_read_261_L%d" % level, level, (d, 261), [_B0, _B0 + 261, _N0], "literal")
        _add("fast_events", "read261_L%d" % level, "out", "fast_read_262_L%d" % level, level, (d, 262), [_B0, _B0 + 262, _N0], "sweeps")
    for level in (2, 3):  # a Write end against the slide threshold (level 1: the slide family), the read capped by the window's room
        for pair, edge in zip(_SLIDE_PAIRS, ("threshold_lo", "threshold_hi", "window_end")):
            d = _slide_data(level, W1, pair)
            for off in pair:
                _add("fast_events", "%s_L%d" % (edge, level), "in" if off in (-262, -2, 0) else "out", "fast_end_%d_L%d" % (W1 + off, level), level, (d, off),
                     [_A0, W1 + off, 100000], "literal" if -262 <= off <= -2 or off == 1 else "sweeps")
    # a match longer than max_insert at the event: its second position is inserted by the event alone
    d = _event_top_data(2)
    for side, end in (("out", _B0), ("in", _B0 - 1)):
        _add("fast_events", "max_insert_L2", side, "fast_insert_%s_L2" % ("behind_match" if side == "out" else "in_match"), 2, (d, side), [_A0, end, _N0], "sweeps")


# ------------------------------------------------------------------ rle_fold
def _rle_data(n):
    def build(seed):
        b = mc._B(seed)
        while len(b) < n:  # runs of 1 to 40 equal bytes
            b.d += bytes([b.rng.choice(mc.ALPHA[:8])]) * b.rng.randrange(1, 40)
        del b.d[n:]
        return b.bytes(), {None: None}
    return build


def _rle_cases():
    d = _rle_data(133000)
    for level in (1, 6):
        for E in (65273, 65274, 65535, 65536, 98041, 98042):
            tail = E >= W1 - LA and E % WS >= WS - LA
            edge = "rle_%d_L%d" % (65274 if E < 65300 else 65536 if E < 70000 else 98042, level)
            _add("rle_fold", edge, "in" if tail else "out", "rle_end_%d_L%d" % (E, level), level, (d, None), [E, 133000], "literal" if tail else "folded", strategy=RLE,
                 route_only=True)


# ------------------------------------------------------------------ resume
_F0 = 30000  # the flushed first Write of the cases that take their Write lists from the cluster and lookahead families


def _flush_slide_data(level):
    """A first Write under a flush mode that ends at 65273 or 65274, the rest one Write; a probe at 65275.  Flushed at 65274 the
    engine stands on the slide threshold: the flush's own last pass through the loop slides the window, the run behind it
    starts at window index 32506 and its first read inserts 65275 ahead.  Flushed at 65273 the window slides at 65275, the
    window end's event, which finds the probe."""
    def build(seed):
        L = _Layout(seed, 100000)
        L.at(W1 - 275, L.high(13))
        pr = L.probe(W1 - 261, W1 - 2600)
        data = L.bytes()

        def claim(F):
            def c(t, reads, slides):
                r = reads_at(reads, F)
                return (after(reads, F) == F and slides[0] == (SLIDE_AT if F == SLIDE_AT else SLIDE_AT + 1, WS) and r and r[0][3] == (WS if F == SLIDE_AT else 0) and
                        _hits(t, {pr: 1 if F == SLIDE_AT else 0}))
            return c
        return data, claim
    return build


def _flush_end_data(level):
    """A flush 524 or 523 bytes in front of the stream's end, a probe at n - 523: the run behind the flush goes back to the
    parallel forms when it has 524 bytes (262 loop-tops with a full lookahead) and stays with the literal engine when not."""
    def build(seed):
        L = _Layout(seed, _N0)
        L.at(_N0 - 537, L.high(13))
        pr = L.probe(_N0 - 523, _N0 - 3000)
        data = L.bytes()

        def claim(F):
            def c(t, reads, slides):
                return after(reads, F) == F and _hits(t, {pr: 1 if F == _N0 - 524 else 0})
            return c
        return data, claim
    return build


def _resume_cases():
    for level in (6, 1):
        d = _flush_slide_data(level)
        for F, side in ((SLIDE_AT - 1, "out"), (SLIDE_AT, "in")):
            _add("resume", "at_read_p0_L%d" % level, side, "resume_flush_at_%d_L%d" % (F, level), level, (d, F), [F, 100000], "resumed", flushes=[2, 0])
    for level in (6, 4, 1, 3):
        d = _flush_end_data(level)
        for F, side, route in ((_N0 - 524, "in", "resumed"), (_N0 - 523, "out", "literal")):
            _add("resume", "run_of_524_L%d" % level, side, "resume_flush_%d_before_the_end_L%d" % (_N0 - F, level), level, (d, F), [F, _N0], route, flushes=[2, 0])
    # the Write lists of the cluster and lookahead families behind a flushed first Write (Sync; Full at level 4)
    for level, gap_in in ((6, 270), (4, 262)):
        d = _cluster_data(level, gap_in)
        for gap in (gap_in, gap_in + 1):
            _add("resume", "gap%d_L%d" % (gap_in, level), "in" if gap == gap_in else "out", "resume_gap_%d_L%d" % (gap, level), level, (d, gap),
                 [_F0, _B0, _B0 + gap, _N0], "resumed", flushes=[3 if level == 4 else 2, 0, 0, 0])
    d, la = _lookahead_data(6)
    for side, w in (("in", 261 - la), ("out", 262 - la)):
        _add("resume", "w261_L6", side, "resume_ahead_%d_L6" % (la + w), 6, (d, ("w261", side)), [_F0, _B0, _B0 + w, _N0], "resumed", flushes=[2, 0, 0, 0])
    for side, third in (("in", 100), ("out", 262 - la - 4)):
        _add("resume", "chain_L6", side, "resume_chain_%s_L6" % ("one_top" if side == "in" else "two_tops"), 6, (d, ("chain", side)),
             [_F0, _B0, _B0 + 1, _B0 + 4, _B0 + 4 + third, _B0 + 4 + third + 261, _N0], "resumed", flushes=[2, 0, 0, 0, 0, 0, 0])
    d = _fast_read_data(1)
    _add("resume", "read261_L1", "in", "resume_read_261_L1", 1, (d, 261), [_F0, _B0, _B0 + 261, _N0], "literal", flushes=[2, 0, 0, 0])
    _add("resume", "read261_L1", "out", "resume_read_262_L1", 1, (d, 262), [_F0, _B0, _B0 + 262, _N0], "resumed", flushes=[2, 0, 0, 0])


# ------------------------------------------------------------------ the catalogue
_event_top_cases()
_lookahead_cases()
_cluster_cases()
_slide_cases()
_tail_cases()
_poison_cases()
_fast_cases()
_rle_cases()
_resume_cases()

# seeds tuned on the CPU until the claims of all the cases that share the bytes held (the default is 1): accidental
# bucket-mates of the filler, mostly
_SEEDS = {"slide_nil_98304_dist32506_L6": 4, "slide_nil_98304_dist32505_L6": 4, "slide_nil_98304_dist32506_L1": 4, "slide_nil_98304_dist32505_L1": 4}

FAMILY_COUNTS = {}
for _m in META.values():
    FAMILY_COUNTS[_m[0]] = FAMILY_COUNTS.get(_m[0], 0) + 1


def case_names(family=None):
    """The catalogue's names without building it (for parametrised tests)."""
    return [s[0] for s in _SPECS if family is None or META[s[0]][0] == family]


_DATA = {}


@functools.lru_cache(maxsize=None)
def case(name, seed=None):
    name_, level, strategy, ends, route, (build, key), flushes = next(s for s in _SPECS if s[0] == name)
    seed = _SEEDS.get(name, 1) if seed is None else seed
    if (build, seed) not in _DATA:
        _DATA[(build, seed)] = build(seed)
    data, claims = _DATA[(build, seed)]
    claim = claims(key) if callable(claims) else claims[key]
    assert ends[-1] == len(data) and list(ends) == sorted(set(ends)), name
    return name, data, level, strategy, list(ends), flushes, claim, route


def writes(ends):
    """Write sizes of cumulative ends"""
    return [ends[0]] + [ends[i] - ends[i - 1] for i in range(1, len(ends))]


def twins(name):
    """the cases on the other side of `name`'s edge that have the same bytes"""
    family, edge, side = META[name]
    data = case(name)[1]
    return [n for n in case_names(family) if META[n][1] == edge and META[n][2] != side and case(n)[1] == data]


def catalogue():
    return tuple(case(n) for n in case_names())


# ------------------------------------------------------------------ the oracle's word on a case, made once (for both test files)
_TRACES = {}
_SINGLE = {}


def trace(oracle, name):
    """(stream, tokens, reads, slides) of a case's schedule on the oracle"""
    import deflate_reader as dr
    if name not in _TRACES:
        _, data, level, strategy, ends, flushes, _, _ = case(name)
        z, reads, slides = oracle.trace(data, level, strategy, writes(ends), flushes)
        want = oracle.compress_writes(data, level, strategy, writes(ends), flushes) if flushes else oracle.compress(data, level, strategy, chunks=writes(ends))
        assert z == want  # (the trace changes nothing)
        _TRACES[name] = (z, mc.tokens(dr.read(z)), reads, slides)
    return _TRACES[name]


def ref(oracle, name):
    return trace(oracle, name)[0]


def single(oracle, name):
    """the oracle's stream of a case's bytes in one Write"""
    _, data, level, strategy, _, _, _, _ = case(name)
    key = (data, level, strategy)
    if key not in _SINGLE:
        _SINGLE[key] = oracle.compress(data, level, strategy)
    return _SINGLE[key]


# The hash_variant = 1 leg (the event_top and slide families).  The probes and the planted matches are found by content under
# either hash; the claims that count a bucket's members (eq_bucket, nil) do so through the oracle's own hash of that variant.
# Left out by name: the cases whose claim does not survive the multiplicative hash.
NOT_UNDER_HASH_VARIANT_1 = tuple("slide_nil_%d_dist%d_L%d" % (W, d, lv) for lv in (6, 1) for W in (W1, W2) for d in (MAX_DIST, MAX_DIST - 1))
# (the nil cases want the source alone in its bucket, which the seeds give them under the reference's CRC-32C)


def hash_variant_names():
    return [n for n in case_names() if META[n][0] in ("event_top", "slide") and n not in NOT_UNDER_HASH_VARIANT_1]


def takes_hash_variant(name):
    """the claim counts bucket members: it is called as claim(tokens, reads, slides, hash_variant)"""
    return META[name][1].startswith(("eq_bucket", "nil"))

