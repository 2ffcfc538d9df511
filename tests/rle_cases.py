"""Inputs for CompressionStrategy.Rle on one NoFlush Write -- KR: the formulation of zs_rle.h (rle_role, rle_body_end,
rle_refills_fired_at), the five launches of zs_rle.hip and the hand-over to the literal engine -- at the edges of its runs, its
tiles and its hand-over, which the corpus and random run lengths meet only by chance.

A case is (name, data, level, writes, claim).  `writes` is None: every case is one Write (two_writes() below cuts a case for the
legs that fold a Write list).  The claim is a predicate over the ORACLE's stream of the case -- claim(t, blocks, slides) with t the
tokens of match_cases.tokens ({position: (length, distance)}, a literal is (1, 0)), blocks what deflate_reader.read returns and
slides oracle.trace's [(loop-top, new window base)] -- and says which side of its rule's edge the case is on.
tests/test_rle_cases.py holds every claim against the oracle on the CPU and runs every case through the CPU model;
tests/test_gpu_rle_cases.py then asks the device for the oracle's bytes.  A claim is never evaluated on the device's stream.

parse(data) is Deflate.Rle.cs:26-98 restated: one loop-top after another, the match the run of the byte before.  It is the
reference the claims use where they say "the tokens here".

The filler is bytes over 64 values whose neighbours all differ: every token outside the constructed runs is a literal.  The runs'
bytes are values the filler does not have.  Everything is generated from frozen seeds.

META[name] = (family, edge, side): every edge of every family has cases on both of its sides ("placement" has no far side: it
is the slot shapes moved over the device's grids), which test_rle_cases.py counts.  slot_start(name) is a `measure` case's slot
start and the residue modulo 8 that its address must have on the device (the position has that residue itself: the GPU test places
the input at an address that is a multiple of 8)."""
import functools
import random

RLE = 3
MIN_MATCH, MAX_MATCH, W, WINDOW, BLOCK_SYMS, TILE = 3, 258, 32768, 65536, 16383, 4096
SEG0 = WINDOW - MAX_MATCH  # kRleSeg0: the first refill's trigger
PIECE = 1024 * TILE        # positions per piece of zs_rle_scan_kernel and zs_rle_sums_kernel
ALPHA = bytes(range(0x40, 0x80))
A, B, C = 0x01, 0x02, 0x03  # the runs' bytes


def trigger(k):
    """the loop-top from which refill k >= 1 of a single Write has fired"""
    return SEG0 + W * (k - 1)


def body_end(n):
    """rle_body_end (zs_rle.h) restated: n - 786, moved below a trigger that lies within 258 of it; -1: no body"""
    h = n - 3 * 262
    moved = True
    while moved and h > 0:
        moved = False
        t = SEG0
        while t <= h:
            if t > h - MAX_MATCH:
                h, moved = t - MAX_MATCH - 1, True
            t += W
    return h if h >= 4096 else -1


def parse(data):
    """{loop-top: (length, distance)} by Deflate.Rle.cs: a match needs three bytes ahead and a byte before"""
    n, s, out = len(data), 0, {}
    while s < n:
        ahead = data[s:s + MAX_MATCH]
        length = len(ahead) - len(ahead.lstrip(data[s - 1:s])) if s > 0 and n - s >= MIN_MATCH else 0
        out[s] = (length, 1) if length >= MIN_MATCH else (1, 0)
        s += length if length >= MIN_MATCH else 1
    return out


def run_tokens(a, L):
    """the tokens of a run of L bytes at a behind another byte: a literal, q matches of 258, then nothing, one literal, two
    literals or one match of r"""
    q, r = divmod(L - 1, MAX_MATCH)
    out = {a: (1, 0)}
    for j in range(q):
        out[a + 1 + MAX_MATCH * j] = (MAX_MATCH, 1)
    at = a + 1 + MAX_MATCH * q
    if r >= MIN_MATCH:
        out[at] = (r, 1)
    else:
        for j in range(r):
            out[at + j] = (1, 0)
    return out


def has(t, want, lo, hi):
    """the tokens in [lo, hi) are exactly `want`'s there"""
    return {p: v for p, v in t.items() if lo <= p < hi} == {p: v for p, v in want.items() if lo <= p < hi}


@functools.lru_cache(maxsize=4)
def _filler(seed):
    rng = random.Random(seed)
    d = bytearray(rng.choices(ALPHA, k=140 << 10))
    for i in range(1, len(d)):
        if d[i] == d[i - 1]:
            d[i] = ALPHA[(d[i] - 0x40 + 1 + rng.randrange(62)) % 64]
    return bytes(d)


@functools.lru_cache(maxsize=4)
def _noise(seed):
    """... over the 255 values but 0: with the end-of-block code and a length code the tree has more than 256 leaves, some of nine
    bits, and a block of it goes stored"""
    rng = random.Random(seed)
    d = bytearray(rng.choices(range(1, 256), k=40000))
    for i in range(1, len(d)):
        if d[i] == d[i - 1]:
            d[i] = 1 + (d[i] + rng.randrange(253)) % 255
    return bytes(d)


class _B:
    def __init__(self, seed, noise=False):
        self.f, self.at, self.d = _noise(seed) if noise else _filler(seed), 0, bytearray()

    def __len__(self):
        return len(self.d)

    def fill(self, n):
        assert n >= 0 and self.at + n <= len(self.f), (n, self.at)
        if n and self.d and self.d[-1] == self.f[self.at]:
            self.at += 1
        self.d += self.f[self.at:self.at + n]
        self.at += n
        return self

    def fill_to(self, n):
        return self.fill(n - len(self.d))

    def run(self, L, byte=A):
        assert not self.d or self.d[-1] != byte
        p = len(self.d)
        self.d += bytes([byte]) * L
        return p

    def absorb(self, shift):
        """runs of 1 + m bytes (two symbols each) so that the symbols behind lie `shift` positions further on than their number"""
        byte = B
        while shift > 0:
            m = min(MAX_MATCH, shift + 1)
            if shift + 1 - m == 1:
                m -= 1
            if m < MIN_MATCH:
                m = MIN_MATCH
            self.run(1 + m, byte)
            shift -= m - 1
            byte = B + C - byte
        assert shift == 0
        return self

    def short_runs(self, nbytes, rng):
        """runs of 1 to 40 bytes over four values: thousands of symbols"""
        end = len(self.d) + nbytes
        while len(self.d) < end:
            byte = rng.choice([v for v in (0x10, 0x11, 0x12, 0x13) if not self.d or v != self.d[-1]])
            self.run(min(rng.randint(1, 40), end - len(self.d)), byte)
        return self

    def bytes(self):
        return bytes(self.d)


_SPECS = []
META = {}
AT = {}
_SLOT_START = {}
LEVEL = 6


def _add(family, edge, side, name, build):
    assert name not in META, name
    META[name] = (family, edge, side)
    _SPECS.append((name, build))


# ------------------------------------------------------------------ slot (rle_role)
SLOT_LENGTHS = (1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 263, 516, 517, 518, 519, 520, 521, 774, 775)


def _slot_case(L, a=1000, total=6000, again=None):
    """a run of L bytes at a behind a different byte (a = 0: at the stream's start); again: the same byte's run once more, one
    foreign byte behind the first"""
    def build(seed):
        b = _B(seed).fill(a)
        s = b.run(L)
        if again:
            b.fill(1)
            s2 = b.run(again)
        b.fill_to(total)
        data = b.bytes()

        def claim(t, blocks, slides):
            if again:
                return has(t, {**run_tokens(s, L), s + L: (1, 0), **run_tokens(s2, again)}, s, s2 + again) and t.get(s2 + again) == (1, 0)
            return has(t, run_tokens(s, L), s, s + L) and t.get(s + L) == (1, 0)
        return data, claim
    return build


def _slot_side(L):
    q, r = divmod(L - 1, MAX_MATCH)
    if r == 257 or (r == 0 and q):
        return "full_slot", "in" if r == 257 else "out"
    return "min_match_q%d" % q, "in" if r >= MIN_MATCH else "out"


def _slot_cases():
    for L in SLOT_LENGTHS:
        edge, side = _slot_side(L)
        _add("slot", edge, side, "slot_run_%d" % L, _slot_case(L))
    for L in (3, 4, 259, 260):  # position 0 is always a literal, the match starts at 1
        _add("slot", "position0", "in" if (L - 1) % MAX_MATCH >= MIN_MATCH else "out", "slot_at_0_run_%d" % L, _slot_case(L, a=0))
    for L, L2 in ((5, 3), (5, 4), (260, 3), (260, 263)):
        _add("slot", "same_byte_again", "in" if L2 > 3 else "out", "slot_again_%d_%d" % (L, L2), _slot_case(L, again=L2))


# ------------------------------------------------------------------ measure (the run measure of zs_rle_pass_kernel)
MEASURE_LEFT = (1, 2, 3, 7, 8, 9, 15, 16, 17, 255, 256, 257, 258, 259, 263, 264, 265, 300)


def _measure_case(left, residue):
    """`left` bytes of the run from its first slot start on, the slot start at `residue` modulo 8; one foreign byte behind the
    run and the run's own byte again, so that only the first mismatch of a load may count"""
    def build(seed):
        a = 1000 + (residue - 1001) % 8
        b = _B(seed).fill(a)
        s = b.run(1 + left)
        b.fill(1)
        s2 = b.run(20)
        b.fill_to(5200)
        data = b.bytes()
        assert (s + 1) % 8 == residue and body_end(len(data)) > s2 + 40

        def claim(t, blocks, slides):
            want = (min(left, MAX_MATCH), 1) if left >= MIN_MATCH else (1, 0)
            return t.get(s + 1) == want and has(t, run_tokens(s, 1 + left), s, s + 1 + left) and t.get(s2 + 1) == (19, 1)
        _SLOT_START[(left, residue)] = s + 1
        return data, claim
    return build


def _measure_cases():
    for left in MEASURE_LEFT:
        if left <= 3:
            edge, side = "min_match", "in" if left >= MIN_MATCH else "out"
        elif left <= 17:
            step = 8 if left <= 9 else 16
            edge, side = "load_%d" % step, "in" if left < step else "out"
        else:
            edge, side = "cap_258", "in" if left <= MAX_MATCH else "out"
        for residue in range(8):
            name = "measure_left_%d_at_%d_mod_8" % (left, residue)
            _add("measure", edge, side, name, _measure_case(left, residue))
            AT[name] = (left, residue)


# ------------------------------------------------------------------ placement (the device's grids)
def _place_case(a, L, lead=None):
    """the run of L bytes at a; lead: another run from that position up to a (no run start between the two)"""
    def build(seed):
        b = _B(seed)
        if lead is not None:
            b.fill(lead)
            b.run(a - lead, B)
        else:
            b.fill(a)
        s = b.run(L)
        assert s == a
        b.fill_to(max(a + L + 1200, 6000))
        data = b.bytes()
        assert body_end(len(data)) > a + L + 300

        def claim(t, blocks, slides):
            ok = has(t, run_tokens(a, L), a, a + L) and t.get(a + L) == (1, 0)
            return ok and (lead is None or has(t, run_tokens(lead, a - lead), lead, a))
        return data, claim
    return build


def _placements():
    out = []
    for a in (4160, 4223, 4095, 4096):  # the run start on lane 0, on lane 63, on a tile's last position, on its first
        for L in (3, 4, 260):
            out.append(("start", a, L, None))
    for at in (4223, 4095):  # the slot start (k == 0) there: the first slot, and the second
        out.append(("slot_k0", at - 1, 2, None))
        out.append(("slot_k0", at - 1, 300, None))
        out.append(("slot_k0", at - 1 - MAX_MATCH, 262, None))
        out.append(("slot_k0", at - 1 - MAX_MATCH, 259 + 258, None))
    for at in (4223, 4095, 8191):  # the literal behind a short slot (k == 1) there
        out.append(("slot_k1", at - 2, 3, None))
        out.append(("slot_k1", at - 2 - MAX_MATCH, 261, None))
    for tiles in (1, 2, 3):  # whole tiles without a run start: `last` is -1 for them
        out.append(("whole_tiles_%d" % tiles, 4000, TILE * tiles + 200, None))
        out.append(("whole_tiles_%d" % tiles, 4095, TILE * tiles + 2, None))
    for a in (8191, 12287):  # a tile's first run start on its last lane (the run before it began in tile 0)
        out.append(("first_start_last_lane", a, 300, 3000))
        out.append(("first_start_last_lane", a, 2, 3000))
    return out


def _place_cases():
    for tag, a, L, lead in _placements():
        _add("placement", "place", "in", "place_%s_%d_run_%d" % (tag, a, L), _place_case(a, L, lead))


# ------------------------------------------------------------------ pieces (the scan's and the sums' 1024 tiles)
def _pieces_case(kind):
    def build(seed):
        rng = random.Random(seed)
        b = _B(seed).fill(100 if kind == "whole_piece" else 3000)
        if kind == "whole_piece":  # a run from 100 to behind the third piece's start: the second has no run start
            marks = [b.run(2 * PIECE + 5000 - 100)]
        elif kind == "cross":
            b.run(PIECE - 1000 - len(b), B)
            marks = [b.run(2000)]
        else:
            at = PIECE - 1 if kind == "start_4194303" else PIECE
            b.run(at - len(b), B)
            marks = [b.run(700)]
        marks.append(len(b))
        b.short_runs(60000, rng)
        b.fill(1000)
        data = b.bytes()

        def claim(t, blocks, slides):
            want = parse(data)
            ok = all(has(t, want, m - 600, m + 1500) for m in marks) and has(t, want, len(data) - 3000, len(data))
            for edge in (PIECE, 2 * PIECE):
                if edge < len(data):
                    ok = ok and has(t, want, edge - 600, edge + 600)
            return ok and t.get(marks[0]) == (1, 0) and t.get(marks[0] + 1) == (MAX_MATCH, 1)
        return data, claim
    return build


def _pieces_cases():
    _add("pieces", "piece_start", "in", "pieces_start_4194303", _pieces_case("start_4194303"))
    _add("pieces", "piece_start", "out", "pieces_start_4194304", _pieces_case("start_4194304"))
    _add("pieces", "piece_carry", "in", "pieces_run_across_4194304", _pieces_case("cross"))
    _add("pieces", "piece_carry", "out", "pieces_run_100_to_behind_8388608", _pieces_case("whole_piece"))


# ------------------------------------------------------------------ block_cut (blk_end / blk_top every 16 383 symbols)
def _cut_case(kind, at=None, stored=False):
    """symbol number 16 383 is a literal, a match of 3 or a match of 258; at: its position (runs in front move it there); stored:
    among bytes over 255 values, so that the block behind the cut goes stored -- and the one in front of it, unless it ends in
    the match of 258 -- and blk_end is where the stored bytes are cut"""
    def build(seed):
        b = _B(seed, stored).fill(500)
        if at is not None:
            b.absorb(at - (BLOCK_SYMS - 1))
        nsyms = len(parse(b.bytes()))  # so far: 500 literals and two per absorbing run
        front = BLOCK_SYMS - 1 - nsyms - (0 if kind == "lit" else 1)
        b.fill(front)
        p = len(b) if kind == "lit" else len(b) + 1
        if kind == "lit":
            b.fill(1)
        else:
            b.run(4 if kind == "m3" else 259, 0 if stored else A)
        assert at is None or p == at, (p, at)
        b.fill_to(max(len(b) + 2000, 20000))
        data = b.bytes()
        assert body_end(len(data)) > len(data) - 800

        def claim(t, blocks, slides):
            want = {"lit": (1, 0), "m3": (3, 1), "m258": (258, 1)}[kind]
            if stored:  # (a match of 258 as its last symbol is what keeps the first block from going stored)
                first = blocks[0].symbols[-1] == want if kind == "m258" else blocks[0].kind == "stored" and blocks[0].len == p + want[0]
                return first and len(blocks) == 2 and blocks[1].kind == "stored" and blocks[1].len == len(data) - (p + want[0])
            last = blocks[0].symbols[-1]
            return len(blocks[0].symbols) == BLOCK_SYMS and t.get(p) == want and (last.__class__ is int) == (kind == "lit") and \
                sorted(t)[BLOCK_SYMS - 1] == p
        return data, claim
    return build


def _body_syms_case(k, d):
    """filler alone: n = 16 383 k + 786 + d has H = 16 383 k + d, a symbol per position"""
    def build(seed):
        data = _B(seed).fill(BLOCK_SYMS * k + 786 + d).bytes()
        assert body_end(len(data)) == BLOCK_SYMS * k + d

        def claim(t, blocks, slides):
            counts = [len(b.symbols) for b in blocks]
            return counts == [BLOCK_SYMS] * k + [786 + d] and all(v == (1, 0) for v in t.values())
        return data, claim
    return build


def _cut_cases():
    for kind in ("lit", "m3", "m258"):
        side = "out" if kind == "lit" else "in"
        _add("block_cut", "cut_symbol", side, "cut_%s" % kind, _cut_case(kind))
        _add("block_cut", "cut_symbol_lane_63", side, "cut_%s_on_lane_63" % kind, _cut_case(kind, 16447))
        _add("block_cut", "cut_symbol_tile_last", side, "cut_%s_on_tile_last" % kind, _cut_case(kind, 5 * TILE - 1))
        _add("block_cut", "cut_symbol_stored", side, "cut_%s_in_front_of_a_stored_block" % kind, _cut_case(kind, stored=True))
    for k in (1, 2):
        for d in (-1, 0, 1):  # the literal engine starts inside the open block, right behind a closed one, one symbol into the next
            _add("block_cut", "body_syms_%d" % k, "out" if d < 0 else "in", "cut_body_syms_%dx16383%+d" % (k, d), _body_syms_case(k, d))


# ------------------------------------------------------------------ handover (rle_body_end, ph, k_done)
def _handover_case(n, kind):
    """kind: "filler"; "run": one run from H - 600 to H + 600; "m258_at_H-1": a match of 258 begins at H - 1, ph = H + 257;
    "top_on_H": a slot start on H"""
    def build(seed):
        H = body_end(n)
        Hx = H if H >= 0 else n - 786
        b = _B(seed)
        if kind == "filler":
            pass
        elif kind == "run":
            b.fill(Hx - 600).run(1200)
        else:
            slot = Hx - 1 if kind == "m258_at_H-1" else Hx
            a = slot - 1 - MAX_MATCH
            b.fill(a).run(1 + MAX_MATCH + MAX_MATCH + 5)
        b.fill_to(n)
        data = b.bytes()

        def claim(t, blocks, slides):
            want = parse(data)
            ok = has(t, want, Hx - 300, n)
            if kind == "m258_at_H-1":
                ok = ok and t.get(Hx - 1) == (MAX_MATCH, 1) and Hx not in t
            if kind == "top_on_H":
                ok = ok and t.get(Hx) == (MAX_MATCH, 1)
            if kind == "filler":
                ok = ok and all(v == (1, 0) for v in t.values())
            tops = sorted(t)
            k = 1
            while trigger(k) + MAX_MATCH < n:  # refill k: more data lies behind the window's end
                first = next(p for p in tops if p >= trigger(k))
                ok = ok and len(slides) >= k and slides[k - 1] == (first, W * k)
                k += 1
            return ok and len(slides) == k - 1
        return data, claim
    return build


HANDOVER_KINDS = ("filler", "run", "m258_at_H-1", "top_on_H")


def _handover_cases():
    for n, side in ((4881, "out"), (4882, "in")):
        for kind in ("filler", "run"):
            _add("handover", "shortest_body", side, "handover_n%d_%s" % (n, kind), _handover_case(n, kind))
    for k in (1, 2, 3):
        t = trigger(k)
        for d, side in ((-1, "out"), (0, "in"), (257, "in"), (258, "out")):  # H = t - 1, t - 259, t - 259, t + 258
            for kind in HANDOVER_KINDS:
                _add("handover", "trigger_%d" % k, side, "handover_t%d%+d_%s" % (k, d, kind), _handover_case(t + d + 786, kind))
    for kind in ("run", "m258_at_H-1"):  # H = 8191: the hand-over loop-top lies in the tile behind H's
        _add("handover", "tile_behind", "in", "handover_h8191_%s" % kind, _handover_case(8192 + 785, kind))
    _add("handover", "tile_behind", "out", "handover_h8191_filler", _handover_case(8192 + 785, "filler"))


# ------------------------------------------------------------------ stored
def _stored_case(with_run):
    def build(seed):
        d = bytearray(random.Random(seed).randbytes(300000))
        if with_run:
            d[130000:170000] = bytes([A]) * 40000
        data = bytes(d)

        def claim(t, blocks, slides):
            kinds = [b.kind for b in blocks]
            if not with_run:
                return set(kinds) == {"stored"} and len(slides) == 8
            other = [i for i, k in enumerate(kinds) if k != "stored"]
            return kinds[0] == kinds[-1] == "stored" and other and other == list(range(other[0], other[-1] + 1)) and len(slides) == 8
        return data, claim
    return build


def _stored_cases():
    _add("stored", "stored", "in", "stored_random_300000", _stored_case(False))
    _add("stored", "stored", "out", "stored_random_300000_run_40000", _stored_case(True))


# ------------------------------------------------------------------ the catalogue
_slot_cases()
_measure_cases()
_place_cases()
_pieces_cases()
_cut_cases()
_handover_cases()
_stored_cases()

FAMILY_COUNTS = {"slot": 27, "measure": 144, "placement": 36, "pieces": 4, "block_cut": 18, "handover": 55, "stored": 2}


def case_names(family=None):
    """The catalogue's names without building it (for parametrised tests)."""
    return [s[0] for s in _SPECS if family is None or META[s[0]][0] == family]


def small_names():
    """every case but the `pieces` family: the streams of 300 000 bytes and less"""
    return [n for n in case_names() if META[n][0] != "pieces"]


@functools.lru_cache(maxsize=None)
def case(name):
    build = next(s[1] for s in _SPECS if s[0] == name)
    data, claim = build(1)
    return name, data, LEVEL, None, claim


def slot_start(name):
    """a `measure` case's slot start and the residue modulo 8 its address must have"""
    case(name)
    return _SLOT_START[AT[name]], AT[name][1]


def two_writes(name):
    """The case as two Writes, the first's end at a seeded position that is not within 262 below a window end (fold_rle_writes
    then folds the list into the single Write)."""
    n = len(case(name)[1])
    rng = random.Random(name)
    while True:
        e = rng.randrange(1, n)
        if not (e >= WINDOW - 262 and e % W >= W - 262):
            return [e, n - e]
