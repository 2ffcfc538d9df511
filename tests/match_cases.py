"""Inputs for the encoder's front end -- the links (K1), the match search (K2), the maps and the speculative walk (K3-K5), the
tail engine (K6) and, for levels 1-3, the sweeps, the runs' engine and fs_search -- at the edges of the reference's rules, which
the corpus, the generators and the fuzzers meet only by chance.

A case is (name, data, level, strategy, writes, claim).  `writes` is None or a list of Write sizes.  The claim is a predicate over
the tokens of the ORACLE's stream of that input (tokens() below: {position: (length, distance)}, a literal is (1, 0)): it says
which side of its rule's edge the case is on.  tests/test_match_cases.py holds every claim against the oracle on the CPU and runs
every case through the CPU model; tests/test_gpu_match_cases.py then asks the device for the oracle's bytes.  A claim is never
evaluated on the device's stream.

The reference hashes the four bytes at p + 2 .. p + 5 (oracle/zs_oracle.c insert_string), so what Longest_match finds by content is
six bytes long or longer; a match of 3 or 4 bytes exists between strings whose hashed bytes differ and share a bucket (_CA, _CB and
_CC do under the reference's CRC-32C; a pair that differs in its last byte alone never does, the CRC being linear: no 5 by
collision), or under the lookahead clip at the end of the input.

The filler is random bytes over 64 values: nothing in it repeats for six bytes, no block goes stored, and the tokens stay visible.
It has accidental bucket-mates though -- about two of three buckets get one within 32 Ki positions -- so a claim that says "the
Nth candidate" or "the head of its bucket" counts the bucket's members itself (mates()), through the oracle's own hash.  Seeds and
sizes were tuned on the CPU until the claims held (_SEEDS), and are frozen.

META[name] = (family, edge, side): every edge of every family has cases on both of its sides, which test_match_cases.py counts."""
import functools
import random

DEFAULT, FILTERED, HO, RLE, FIXED = 0, 1, 2, 3, 4
MAX_DIST = 32506  # kMaxDist
TOO_FAR = 4096    # kTooFar
# level_cfg of zs_core.h (Deflate.cs:80-98): good_length, max_lazy (max_insert at levels 1-3), nice_length, max_chain
LEVELS = {1: (4, 4, 8, 4), 2: (4, 5, 16, 8), 3: (4, 6, 32, 32), 4: (4, 4, 16, 16), 5: (8, 16, 32, 32), 6: (8, 16, 128, 128),
          7: (8, 32, 128, 256), 8: (32, 128, 258, 1024), 9: (32, 258, 258, 4096)}
ALPHA = bytes(range(0x40, 0x80))
_CA, _CB, _CC = b"\x63\x31\x32\x33", b"\x63\xee\xed\xdd", b"\x63\x31\x7f\xa3"  # one bucket; _CA / _CB share 1 byte, _CA / _CC 2

_ORACLE = None


def _hash(v, hv):
    global _ORACLE
    if _ORACLE is None:
        import oracle_binding
        _ORACLE = oracle_binding.Oracle()
    return _ORACLE.L.zso_hash_u32(v, hv) & 32767


# ------------------------------------------------------------------ tokens and buckets
def tokens(blocks):
    """deflate_reader.read(z) as {position: (length, distance)}; a literal -- and a stored block's byte -- is (1, 0)."""
    out, pos = {}, 0
    for b in blocks:
        if b.kind == "stored":
            for _ in range(b.len):
                out[pos] = (1, 0)
                pos += 1
            continue
        for s in b.symbols:
            if s.__class__ is int:
                out[pos] = (1, 0)
                pos += 1
            else:
                out[pos] = s
                pos += s[0]
    return out


def triples(blocks):
    """... and as (position, length, distance) in stream order (tools/deflate_tokens.py's view)."""
    return [(p, l, d) for p, (l, d) in sorted(tokens(blocks).items())]


def matches(t, lo=0, hi=1 << 30):
    return [(p, l, d) for p, (l, d) in sorted(t.items()) if d and lo <= p < hi]


@functools.lru_cache(maxsize=8)
def _buckets(data, hv):
    padded = data + bytes(8)  # (behind the end of a short stream the window is zero)
    return [_hash(int.from_bytes(padded[p + 2:p + 6], "little"), hv) for p in range(len(data))]


def mates(data, p, lo=None, hv=0):
    """Positions in [lo, p) that share p's bucket, nearest first; lo defaults to the far end of p's reach.  Position 0 is never a
    candidate."""
    b = _buckets(bytes(data), hv)
    lo = max(1, p - MAX_DIST if lo is None else lo)
    return [q for q in range(p - 1, lo - 1, -1) if b[q] == b[p]]


# ------------------------------------------------------------------ building blocks
class _B:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.d = bytearray()

    def __len__(self):
        return len(self.d)

    def fill(self, n):
        self.d += bytes(self.rng.choices(ALPHA, k=n))
        return self

    def fill_to(self, n):
        assert n >= len(self.d), (n, len(self.d))
        return self.fill(n - len(self.d))

    def rand(self, n):
        return bytes(self.rng.choices(ALPHA, k=n))

    def other(self, *avoid):
        return self.rng.choice([v for v in ALPHA if v not in avoid])

    def put(self, bs):
        p = len(self.d)
        self.d += bs
        return p

    def guard(self, dist):
        """a byte that differs from the one `dist` back"""
        self.d.append(self.other(self.d[len(self.d) - dist]))

    def copy(self, length, dist):
        p = len(self.d)
        for _ in range(length):
            self.d.append(self.d[len(self.d) - dist])
        return p

    def plant(self, length, dist):
        """guard, `length` bytes that repeat what lies `dist` back, a byte that ends the repeat; returns the target position"""
        self.guard(dist)
        p = self.copy(length, dist)
        self.guard(dist)
        return p

    def bytes(self):
        return bytes(self.d)


def _decoy(j, hashed):
    """six bytes in the bucket of a string whose bytes 2..5 are `hashed`, with leading bytes no filler has"""
    return bytes([0x80 + (j >> 6), 0x80 + (j & 63)]) + hashed


_SPECS = []
META = {}


def _add(family, edge, side, name, level, build, strategy=DEFAULT, writes=None):
    assert name not in META, name
    META[name] = (family, edge, side)
    _SPECS.append((name, level, strategy, writes, build))


# ------------------------------------------------------------------ distance
def _dist_case(dist, decoy=False, length=258):
    def build(seed):
        b = _B(seed).fill(700)
        src = b.put(b.rand(length))
        if decoy:
            b.fill(9000)
            at = b.put(_decoy(0, bytes(b.d[src + 2:src + 6])))
        b.fill_to(src + dist - 1)
        T = b.plant(length, dist)
        b.fill(300)
        data = b.bytes()

        def claim(t, hv=0):
            m = mates(data, T, T - dist, hv)
            if decoy:
                if m != [at, src]:
                    return False
                if dist < MAX_DIST:
                    return t.get(T) == (length, dist)
                # the source is not the head of its bucket: `cur_match > limit` ends the walk in front of it
                got = matches(t, T - 1, T + 3)
                return T not in [g[0] for g in got] and len(got) == 1 and got[0][2] == dist and got[0][1] == length - (got[0][0] - T)
            if m != [src]:
                return False
            if dist <= MAX_DIST:
                return t.get(T) == (length, dist)
            return not matches(t, T - 1, T + length + 1)
        return data, claim
    return build


def _dist3_case(dist):
    """length 3 at the far edge: _CA's and _CB's strings share a bucket and three bytes.  TOO_FAR drops it at levels 4-9."""
    def build(seed):
        b = _B(seed).fill(500)
        src = b.put(b"ab" + _CA)
        b.fill_to(src + dist)
        T = b.put(b"ab" + _CB)
        b.fill(300)
        data = b.bytes()

        def claim(t, hv=0):
            if mates(data, T, T - dist, hv) != [src]:
                return False
            return t.get(T) == ((3, dist) if dist <= MAX_DIST else (1, 0))
        return data, claim
    return build


def _distance_cases():
    for level in (1, 4, 6, 9):
        for dist, side in ((MAX_DIST - 1, "in"), (MAX_DIST, "in"), (MAX_DIST + 1, "out")):
            _add("distance", "max_dist_L%d" % level, side, "dist_%d_L%d" % (dist, level), level, _dist_case(dist))
    _add("distance", "max_dist_L6", "out", "dist_32768_L6", 6, _dist_case(32768))
    for level in (1, 6):
        _add("distance", "head_only_L%d" % level, "in", "dist_32505_decoy_L%d" % level, level, _dist_case(MAX_DIST - 1, True))
        _add("distance", "head_only_L%d" % level, "out", "dist_32506_decoy_L%d" % level, level, _dist_case(MAX_DIST, True))
    for dist, side in ((MAX_DIST, "in"), (MAX_DIST + 1, "out")):
        _add("distance", "len3_far", side, "dist3_%d_L1" % dist, 1, _dist3_case(dist))


# ------------------------------------------------------------------ TOO_FAR, Filtered
def _too_far_case(dist, kept):
    def build(seed):
        b = _B(seed).fill(300)
        src = b.put(b"ab" + _CA)
        b.fill_to(src + dist)
        T = b.put(b"ab" + _CB)
        b.fill(300)
        data = b.bytes()

        def claim(t, hv=0):
            return mates(data, T, T - dist, hv) == [src] and t.get(T) == ((3, dist) if kept else (1, 0))
        return data, claim
    return build


def _end_len5_case(kept):
    """the stream's last five bytes repeat a string whose sixth byte is the zero behind the end: a match cut by the lookahead"""
    def build(seed):
        b = _B(seed).fill(400)
        src = b.put(b"vwxyz\0")
        b.fill(200)
        b.guard(len(b) - src + 1)
        T = b.put(b"vwxyz")
        data = b.bytes()

        def claim(t, hv=0):
            return t.get(T) == ((5, T - src) if kept else (1, 0)) and src in mates(data, T, None, hv)
        return data, claim
    return build


def _len6_case():
    def build(seed):
        b = _B(seed).fill(900)
        T = b.plant(6, 500)
        b.fill(300)
        data = b.bytes()
        return data, lambda t, hv=0: t.get(T) == (6, 500)
    return build


def _too_far_cases():
    for level in (1, 3, 4, 6, 9):
        _add("too_far", "too_far_L%d" % level, "in", "too_far_4096_L%d" % level, level, _too_far_case(TOO_FAR, True))
        _add("too_far", "too_far_L%d" % level, "out", "too_far_4097_L%d" % level, level, _too_far_case(TOO_FAR + 1, level < 4))
    # (levels 1-3 have no TOO_FAR: "out" is the far side of the distance, kept there)
    _add("too_far", "filtered_len", "out", "filtered_len5", 6, _end_len5_case(False), FILTERED)
    _add("too_far", "filtered_len", "in", "filtered_len6", 6, _len6_case(), FILTERED)
    _add("too_far", "filtered_len", "in", "default_len5", 6, _end_len5_case(True))
    _add("too_far", "filtered_len", "out", "filtered_too_far_4096", 6, _too_far_case(TOO_FAR, False), FILTERED)


# ------------------------------------------------------------------ chain budgets
def _budget_case(level, pend, front, long_=None):
    """`front` members of the target's bucket in front of the true source, each rejected by the first-two-bytes test (the near
    source's p + 1 is one of them when a match of `pend` bytes is pending: every bucket-mate counts).  The source is found when
    front < budget: max_chain, or max_chain >> 2 once the pending match is good_length long."""
    good, lazy, nice, chain = LEVELS[level]
    budget = chain >> 2 if pend >= good else chain
    long_ = long_ or (66 if not pend else pend + 12)
    assert long_ < nice or level >= 8, (level, long_)

    def build(seed):
        b = _B(seed).fill(300)
        Z = b.rand(long_)
        c = b.other()
        b.d.append(b.other(c))
        far = b.put(Z)
        b.d.append(b.other())
        ndec = front - (1 if pend else 0)
        for j in range(ndec):
            b.put(_decoy(j, Z[2:6]))
            b.fill(1)
        b.fill(40)
        near = None
        if pend:  # the near source: c and pend - 1 bytes of Z, then a byte that ends the match
            near = b.put(bytes([c]) + Z[:pend - 1])
            b.d.append(b.other(Z[pend - 1]))
            b.fill(40)
        b.d.append(b.other(b.d[far - 1], b.d[near - 1] if pend else c))
        if pend:
            p = b.put(bytes([c]))
        T = b.put(Z)
        b.d.append(b.other(b.d[far + long_]))
        b.fill(300)
        data = b.bytes()
        assert T - far < MAX_DIST

        def claim(t, hv=0):
            m = mates(data, T, far, hv)
            if len(m) != front + 1 or m[-1] != far or (pend and m[0] != near + 1):
                return False
            if pend and t.get(p - 1) != (1, 0):
                return False
            if front < budget:
                return t.get(T) == (long_, T - far) and (not pend or t.get(p) == (1, 0))
            if pend:
                return t.get(p) == (pend, p - near)
            return t.get(T) == (1, 0) and t.get(T + 1) == (long_ - 1, T - far)
        return data, claim
    return build


def _budget_cases():
    for level in range(1, 10):
        good, lazy, nice, chain = LEVELS[level]
        long_ = 7 if level == 1 else 12 if level in (2, 4) else 24 if level in (3, 5) else None
        _add("budget", "chain_L%d" % level, "in", "chain_L%d_front%d" % (level, chain - 1), level, _budget_case(level, 0, chain - 1, long_))
        _add("budget", "chain_L%d" % level, "out", "chain_L%d_front%d" % (level, chain), level, _budget_case(level, 0, chain, long_))
    # the quarter budget (levels 5-9; at level 4 a pending match of good_length is one of max_lazy: nothing is searched behind it)
    for level in range(5, 10):
        good, lazy, nice, chain = LEVELS[level]
        q = chain >> 2
        for pend, front, side in ((good, q - 1, "in"), (good, q, "out"), (good - 1, q, "in"), (good - 1, chain - 1, "in"), (good - 1, chain, "out")):
            edge = "quarter_L%d" % level if front <= q else "pending_full_L%d" % level
            _add("budget", edge, side, "quarter_L%d_pend%d_front%d" % (level, pend, front), level, _budget_case(level, pend, front))


# ------------------------------------------------------------------ nice_length
def _nice_case(level, c):
    """a near candidate of c bytes and one of c + 1 bytes behind it: the walk stops at the near one when c >= nice_length"""
    nice = LEVELS[level][2]
    far_len = min(c + 1, 258)

    def build(seed):
        b = _B(seed).fill(200)
        X = b.rand(259)
        e1, e2, e3 = b.rng.sample(list(ALPHA), 3)
        b.d.append(b.other())
        far = b.put(X[:far_len] + bytes([e1]))
        b.fill(150)
        b.d.append(b.other(b.d[far - 1]))
        near = b.put(X[:c] + bytes([b.other(X[c])]))
        b.fill(150)
        b.d.append(b.other(b.d[far - 1], b.d[near - 1]))
        T = b.put(X[:far_len] + bytes([e3]))
        b.fill(300)
        data = b.bytes()

        def claim(t, hv=0):
            if mates(data, T, far, hv) != [near, far]:
                return False
            if c >= nice or far_len == c:
                return t.get(T) == (c, T - near)
            return t.get(T) == (far_len, T - far)
        return data, claim
    return build


def _nice_cases():
    for level in range(1, 10):
        nice = LEVELS[level][2]
        for c in (nice - 1, nice, nice + 1):
            if c <= 258:
                _add("nice", "nice_L%d" % level, "in" if c < nice else "out", "nice_L%d_near%d" % (level, c), level, _nice_case(level, c))


# ------------------------------------------------------------------ max_lazy and the lazy parse's ties
def _lazy_case(level, lens, coll=None):
    """matches of lens[0], lens[1], .. bytes at p, p + 1, ..: string i is the byte before it and its own tail, its source holds it
    alone.  coll: the first match is 3 or 4 bytes long, by collision."""
    good, lazy, nice, chain = LEVELS[level]

    def build(seed):
        b = _B(seed).fill(300)
        k = len(lens)
        if coll:
            head = b"ab" + (_CB if coll == 3 else _CC)
            S = head + b.rand(lens[1] + 1 - 5)
        else:
            S = b.rand(k - 1 + lens[-1] + 1)
        srcs = []
        for i, n in enumerate(lens):
            b.d.append(b.other(S[i - 1] if i else None))
            if coll and i == 0:
                srcs.append(b.put(b"ab" + _CA))
            else:
                srcs.append(b.put(S[i:i + n]))
                b.d.append(b.other(S[i + n] if i + n < len(S) else None))
            b.fill(60)
        b.d.append(b.other(*[b.d[s - 1] for s in srcs]))
        p = b.put(S)
        b.d.append(b.other(*[b.d[s + n] for s, n in zip(srcs[1:], lens[1:])]))
        b.fill(300)
        data = b.bytes()

        def claim(t, hv=0):
            # the parse by the rule: the pending match is emitted unless it is shorter than max_lazy and the next is longer
            i = 0
            while i + 1 < k and lens[i] < lazy and lens[i + 1] > lens[i]:
                i += 1
            want = {p + j: (1, 0) for j in range(i)}
            want[p + i] = (lens[i], p + i - srcs[i])
            return all(t.get(q) == v for q, v in want.items()) and all(srcs[j] in mates(data, p + j, None, hv) for j in range(i + 1))
        return data, claim
    return build


def _lazy_cases():
    for level in range(4, 10):
        lazy = LEVELS[level][1]
        for m in (lazy - 1, lazy, lazy + 1):
            if level == 4:  # 3 and 4 by collision; 5 cannot be had (see above): 6
                m6 = {3: 3, 4: 4, 5: 6}[m]
                _add("max_lazy", "max_lazy_L4", "in" if m6 < lazy else "out", "lazy_L4_first%d" % m6, 4, _lazy_case(4, (m6, 8), coll=m6 if m6 < 6 else None))
            elif m > 258:
                continue
            elif m + 1 <= 258:
                _add("max_lazy", "max_lazy_L%d" % level, "in" if m < lazy else "out", "lazy_L%d_first%d" % (level, m), level, _lazy_case(level, (m, m + 1)))
            else:
                _add("max_lazy", "max_lazy_L%d" % level, "out", "lazy_L%d_first%d" % (level, m), level, _lazy_case(level, (m, m)))
    for level in range(4, 10):
        _add("lazy_tie", "tie", "in", "tie_equal_L%d" % level, level, _lazy_case(level, (10, 10)))
        _add("lazy_tie", "tie", "out" if level > 4 else "in", "tie_longer_L%d" % level, level, _lazy_case(level, (10, 11)))
    # (level 4 keeps the 10: max_lazy is 4 -- its "out" side is lazy_L4_first3)
    for level in (5, 6, 9):
        _add("lazy_tie", "third_L%d" % level, "out", "tie_three_rising_L%d" % level, level, _lazy_case(level, (10, 11, 12)))
        _add("lazy_tie", "third_L%d" % level, "in", "tie_three_flat_L%d" % level, level, _lazy_case(level, (10, 11, 11)))


def _stale_case(dist, with_mate):
    """a 3-byte candidate at p that p + 1 does not improve: Longest_match at p + 1 returns prev_length with match_start as p left
    it, and the TOO_FAR test behind it reads that stale start"""
    def build(seed):
        b = _B(seed).fill(300)
        if with_mate:
            b.put(b"PQ" + _CB[1:] + b"R")
            b.fill(50)
        src = b.put(b"ab" + _CA)
        b.fill_to(src + dist)
        p = b.put(b"ab" + _CB + b"R")
        b.fill(300)
        data = b.bytes()

        def claim(t, hv=0):
            return t.get(p) == (3, dist) and mates(data, p, p - dist, hv) == [src] and bool(mates(data, p + 1, None, hv)) == with_mate
        return data, claim
    return build


def _stale_cases():
    for level in (4, 6):
        _add("lazy_tie", "stale_L%d" % level, "in", "stale_start_4096_L%d" % level, level, _stale_case(TOO_FAR, True))
        _add("lazy_tie", "stale_L%d" % level, "out", "stale_start_4096_alone_L%d" % level, level, _stale_case(TOO_FAR, False))


# ------------------------------------------------------------------ max_insert (levels 1-3)
def _insert_case(level, m):
    """a match of m bytes at q, fresh bytes R behind it, and later the string that begins at the match's third byte: one piece
    when the match's inside was inserted (m <= max_insert), else only R from the first position behind the match"""
    max_insert = LEVELS[level][1]

    def build(seed):
        b = _B(seed).fill(300)
        if m >= 6:
            E = b.put(b.rand(m))
            b.d.append(b.other())
            b.fill(80)
            b.guard(len(b) - E + 1)
            q = b.put(bytes(b.d[E:E + m]))
        else:
            E = b.put(b"ab" + (_CA if m == 4 else _CB))
            b.fill(80)
            q = b.put(b"ab" + (_CC if m == 4 else _CA))
            assert m in (3, 4)
        head = 6 if m < 6 else m
        R = b.rand(40)
        b.put(R)
        b.d.append(b.other())
        b.fill(80)
        b.d.append(b.other(b.d[q + 1]))
        T = b.put(bytes(b.d[q + 2:q + head]) + R)
        b.d.append(b.other(b.d[q + head + 40]))
        b.fill(300)
        data = b.bytes()

        def claim(t, hv=0):
            if t.get(q) != (m, q - E):
                return False
            if m <= max_insert:
                return t.get(T) == (head - 2 + 40, T - (q + 2)) and q + 2 in mates(data, T, None, hv)
            # q + 1 .. q + m - 1 were never inserted: the first inserted source is q + m
            first = T + m - 2
            return all(t.get(x) == (1, 0) for x in range(T, first)) and t.get(first) == (40 + head - m, T - (q + 2))
        return data, claim
    return build


def _insert_end_case(left):
    """Deflate.Fast.cs: the inside of a short match is inserted only while `lookahead >= MIN_MATCH`: a 4-byte match with `left`
    bytes behind it at the end of the input (3: inserted, the hashes read behind the end; 2: not)"""
    def build(seed):
        b = _B(seed).fill(400)
        E = b.put(b"ab" + _CA)
        b.fill(200)
        q = b.put(b"ab" + _CC[:2 + left] if left < 2 else b"ab" + _CC + b.rand(left - 2))
        data = b.bytes()
        assert len(data) == q + 4 + left
        return data, lambda t, hv=0: t.get(q) == (4, q - E) and all(t.get(x) == (1, 0) for x in range(q + 4, len(data)))
    return build


def _insert_cases():
    for level, pair in ((1, (4, 6)), (2, (4, 6)), (3, (6, 7))):
        for m in pair:
            _add("max_insert", "max_insert_L%d" % level, "in" if m <= LEVELS[level][1] else "out", "insert_L%d_match%d" % (level, m), level, _insert_case(level, m))
    _add("max_insert", "max_insert_L1", "in", "insert_L1_match3", 1, _insert_case(1, 3))
    for level in (1, 3):
        _add("max_insert", "insert_end_L%d" % level, "in", "insert_end_left3_L%d" % level, level, _insert_end_case(3))
        _add("max_insert", "insert_end_L%d" % level, "out", "insert_end_left2_L%d" % level, level, _insert_end_case(2))


# ------------------------------------------------------------------ position 0; the end of the input
def _pos0_case(front):
    def build(seed):
        b = _B(seed)
        b.fill(front)
        X = b.put(b.rand(20))
        b.d.append(b.other())
        b.fill(400)
        b.d.append(b.other(b.d[X - 1] if front else None))
        T = b.put(bytes(b.d[X:X + 20]))
        b.d.append(b.other(b.d[X + 20]))
        b.fill(100)
        data = b.bytes()

        def claim(t, hv=0):
            if front:
                return t.get(T) == (20, T - X)
            return t.get(T) == (1, 0) and t.get(T + 1) == (19, T - X)  # position 0 is never a candidate
        return data, claim
    return build


def _end_case(length, total=None):
    """the stream ends `length` bytes into a repeat of an earlier string: the match is clipped to the lookahead.  Lengths 3, 2 and
    1: the hash reads behind the end -- zeros in a short stream, old window contents (the bytes 32768 back from there) in one of
    more than 64 KiB."""
    def build(seed):
        b = _B(seed)
        if total:
            b.fill(total - 3000)
        b.fill(300)
        src = b.put(b.rand(300))
        b.fill(700)
        dist = len(b) + 1 - src
        T = b.plant(length, dist)
        del b.d[-1]
        n = len(b)
        assert n == T + length
        if length < 6:  # the source's bytes behind the match are what the target's hash reads behind the end
            stale = bytes(b.d[n - 32768 + i] for i in range(3)) if n > 65536 else bytes(3)
            b.d[src + length:src + length + 3] = stale
        data = b.bytes()

        def claim(t, hv=0):
            if length < 3:
                return all(t.get(x) == (1, 0) for x in range(T - 1, n))
            return t.get(T) == (length, dist) and (length >= 6 or src in mates(data + (stale if n > 65536 else b""), T, None, hv))
        return data, claim
    return build


def _edge_cases():
    for level in (1, 6):
        _add("position0", "pos0_L%d" % level, "out", "pos0_repeat_L%d" % level, level, _pos0_case(0))
        _add("position0", "pos0_L%d" % level, "in", "pos1_repeat_L%d" % level, level, _pos0_case(1))
        for length in (258, 40, 3, 2, 1):
            _add("end", "end_clip_L%d" % level, "in" if length >= 3 else "out", "end_%d_L%d" % (length, level), level, _end_case(length))
        for length in (3, 2):
            _add("end", "end_stale_L%d" % level, "in" if length >= 3 else "out", "end_%d_at_70000_L%d" % (length, level), level, _end_case(length, 70000))


# ------------------------------------------------------------------ the slide at a Write end
def _slide_case(first):
    """A repeat planted at 32768 and 65274.  One Write: (100, 32506) at 65274.  A first Write that ends at 65535 or 65534 makes the
    window slide at loop-top 65274; SlideHash turns position 32768 into 0, "none", and the pre-insert of 65275 kills the next
    search: the match starts at 65276 / 65277."""
    def build(seed):
        b = _B(seed).fill(32768)
        X = b.put(b.rand(100))
        b.fill_to(65273)
        T = b.plant(100, MAX_DIST)
        assert T == 65274
        b.fill_to(66000)
        data = b.bytes()
        late = {65535: 2, 65534: 3}.get(first, 0)

        def claim(t, hv=0):
            if mates(data, T, X, hv) != [X]:
                return False
            return t.get(T + late) == (100 - late, MAX_DIST) and all(t.get(T + j) == (1, 0) for j in range(late))
        return data, claim
    return build


def _slide_cases():
    for level in (6, 1):
        for first in (None, 65400, 65534, 65535, 65536):
            _add("slide", "write_end_L%d" % level, "out" if first in (65534, 65535) else "in",
                 "slide_%s_L%d" % ("one_write" if first is None else "first%d" % first, level), level, _slide_case(first), writes=None if first is None else [first, 66000 - first])


# ------------------------------------------------------------------ runs
def _run_case(period, length, start, behind):
    """a run of `length` bytes of one period at `start`; behind it either filler and a planted match whose source lies in front of
    the run, or the run once more"""
    def build(seed):
        b = _B(seed).fill(start - 1)
        unit = bytes(b.rng.sample(list(ALPHA), period))
        b.d.append(b.other(unit[-1]))
        s = b.put((unit * (length // period + 1))[:length])
        b.d.append(b.other(unit[length % period]))
        b.fill(200)
        if behind == "again":
            b.d.append(b.other(b.d[s - 1]))
            s2 = b.put(bytes(b.d[s:s + length]))
            b.d.append(b.other(b.d[s + length]))
        else:
            T = b.plant(30, len(b) + 1 - (s - 100))
        b.fill(300)
        data = b.bytes()

        def claim(t, hv=0):
            first = t.get(s + period) == (min(258, length - period), period) and all(t.get(s + j) == (1, 0) for j in range(period))
            if behind == "again":
                return first and any(d > period for _, _, d in matches(t, s2, s2 + length))
            return first and t.get(T) == (30, T - (s - 100))
        return data, claim
    return build


def _run_cases():
    for level in (1, 3, 6, 9):
        for period in (1, 2, 3, 7):
            for k, length in enumerate((258 + 1, 258 + 2, 2 * 258 + 1, 258 + period, 2 * 258 + period + 1)):
                if (k + period + level) % 3 == 0 or (period == 1 and k < 3):
                    _add("runs", "run_L%d" % level, "in", "run_p%d_%d_L%d" % (period, length, level), level, _run_case(period, length, 600 + 37 * k, "plant"))
        # a run that ends one byte before a chunk edge and a tile edge; the same run twice
        _add("runs", "run_L%d" % level, "in", "run_ends_2047_L%d" % level, level, _run_case(1, 700, 2047 - 700, "plant"))
        _add("runs", "run_L%d" % level, "in", "run_ends_16383_L%d" % level, level, _run_case(3, 900, 16383 - 900, "plant"))
        _add("runs", "run_L%d" % level, "out", "run_twice_p1_L%d" % level, level, _run_case(1, 300, 500, "again"))
        _add("runs", "run_L%d" % level, "out", "run_twice_p7_L%d" % level, level, _run_case(7, 600, 500, "again"))


# ------------------------------------------------------------------ placement against the device's grids
PLACE_LEVELS = (1, 3, 6, 9)


def _place_case(T, length, dist, tail=40):
    """a guard byte, one planted match (length, dist) at position T, an ending byte and `tail` - 1 more bytes.  dist >= MAX_DIST:
    the source must be the head of its bucket (the seed sees to it)."""
    def build(seed):
        if length > dist:  # a unit of `dist` bytes, repeated from T on
            b = _B(seed).fill(T - dist - 1)
            unit = bytes(b.rng.sample(list(ALPHA), dist))
            b.d.append(b.other(unit[-1]))
            b.put(unit)
            at = b.copy(length, dist)
            b.guard(dist)
        else:
            b = _B(seed).fill(T - 1)
            at = b.plant(length, dist)
        assert at == T
        if tail == 0:
            del b.d[-1]
        else:
            b.fill(tail - 1)
        data = b.bytes()
        assert len(data) == T + length + tail

        def claim(t, hv=0):
            if length > dist:
                return all(t.get(T - j) == (1, 0) for j in range(1, dist + 1)) and t.get(T) == (min(258, length), dist)
            if T == 65276 and len(data) > 65536:  # Fill_window at loop-top 65275 inserts 65276 ahead: its own search finds itself
                return t.get(T) == (1, 0) and t.get(T + 1) == (length - 1, dist)
            return t.get(T) == (length, dist) and (dist < MAX_DIST or mates(data, T, T - dist, hv) == [T - dist])
        return data, claim
    return build


def _placements():
    """(tag, T, length, dist, tail)"""
    out = []
    for k in (1, 2, 4):  # K1's and K2's tiles
        for d in (-1, 0, 1):
            out.append(("tile", 16384 * k + d, 40, 300, 40))
    for T in (32768, 65536):  # a tile's first position, the source at the far end of kMatchBack
        out.append(("tile_first_far", T, 258, MAX_DIST, 40))
    for T in (16383, 32767, 65535):  # a tile's last position: the compare and the hash read 263 bytes past it
        out.append(("tile_last_near", T, 258, 1, 40))
    for T in (32767 + 16384, 65535):
        out.append(("tile_last_far", T, 258, MAX_DIST, 40))
    for c in (3, 17):  # the chunk grid of one Write
        for d in (-1, 0, 1):
            out.append(("chunk", 2048 * c - 261 + d, 40, 300, 40))
    for T in (5 * 1024 - 261, 5 * 1024, 9 * 512 - 261, 9 * 512, 9 * 512 - 1):  # the speculative grid
        out.append(("spec", T, 40, 300, 600))
    for T in (65273, 65274, 65275, 65276):  # the slide
        out.append(("slide", T, 40, 300, 600))
        out.append(("slide_far", T, 100, 32000, 600))
    for n in (98304, 131072):  # the match ends the stream at a window end
        out.append(("end", n - 258, 258, 300, 0))
        out.append(("end_m1", n - 259, 258, 300, 1))
    for back in (262, 261, 260, 258, 45):  # where the tail engine's records take over from K2's
        out.append(("tail", 40000, 40, 300, back - 40))
    out.append(("src_tile_last", 20000, 40, 20000 - 16383, 40))
    out.append(("src_tile_last_far", 16383 + MAX_DIST, 258, MAX_DIST, 40))
    out.append(("dist_eq_len", 16384, 40, 40, 40))
    out.append(("dist_eq_len", 32767, 258, 258, 40))
    for dist in (1, 2):
        out.append(("near", 16384, 40, dist, 40))
        out.append(("near", 2048 * 8 - 261, 300, dist, 40))
        out.append(("slide_run", 65200, 300, dist, 600))  # the window end's event falls into the run: its loop-top shares its bucket with the next position
    return out


def _place_cases():
    for level in PLACE_LEVELS:
        for tag, T, length, dist, tail in _placements():
            name = "place_%s_%d_%dx%d_t%d_L%d" % (tag, T, length, dist, tail, level)
            _add("placement", "place_L%d" % level, "in", name, level, _place_case(T, length, dist, tail))


# ------------------------------------------------------------------ the catalogue
_distance_cases()
_too_far_cases()
_budget_cases()
_nice_cases()
_lazy_cases()
_stale_cases()
_insert_cases()
_edge_cases()
_slide_cases()
_run_cases()
_place_cases()

# seeds tuned on the CPU until the claim held (the default is 1): accidental bucket-mates of the filler, mostly
_SEEDS = {"dist3_32506_L1": 4, "dist3_32507_L1": 4, "chain_L2_front8": 2, "chain_L9_front4095": 2, "chain_L9_front4096": 2, "slide_first65534_L6": 2,
          "slide_first65534_L1": 2}
for _lv in (1, 3, 6, 9):
    _SEEDS["place_tile_first_far_65536_258x32506_t40_L%d" % _lv] = 3
    _SEEDS["place_tile_last_far_49151_258x32506_t40_L%d" % _lv] = 3
    _SEEDS["place_tile_last_far_65535_258x32506_t40_L%d" % _lv] = 2

# The hash_variant = 1 leg (the distance and budget families): the buckets differ there, so the cases whose filler has a
# bucket-mate in the way under the multiplicative hash are built from another seed for that leg -- the same construction, the same
# claim, which tests/test_match_cases.py holds against the oracle under that variant.  Left out by name: the cases that rest on
# collisions of the reference's CRC-32C.
NOT_UNDER_HASH_VARIANT_1 = ("dist3_32506_L1", "dist3_32507_L1")
_SEEDS_HASH_VARIANT_1 = {"quarter_L9_pend31_front4095": 2, "quarter_L9_pend31_front4096": 2}
_SEEDS_HASH_VARIANT_1.update({n: 6 for n in (["dist_%d_L%d" % (d, lv) for d in (32505, 32506, 32507) for lv in (1, 4, 6, 9)] + ["dist_32768_L6"] +
                                               ["dist_%d_decoy_L%d" % (d, lv) for d in (32505, 32506) for lv in (1, 6)])})

FAMILY_COUNTS = {"distance": 19, "too_far": 14, "budget": 43, "nice": 25, "max_lazy": 17, "lazy_tie": 22, "max_insert": 11, "position0": 4, "end": 14,
                 "slide": 10, "runs": 49, "placement": 216}


def case_names(family=None):
    """The catalogue's names without building it (for parametrised tests)."""
    return [s[0] for s in _SPECS if family is None or META[s[0]][0] == family]


@functools.lru_cache(maxsize=None)
def case(name, seed=None):
    name_, level, strategy, writes, build = next(s for s in _SPECS if s[0] == name)
    data, claim = build(_SEEDS.get(name, 1) if seed is None else seed)
    return name, data, level, strategy, writes, claim


def catalogue():
    return tuple(case(n) for n in case_names())


def hash_variant_names():
    """the distance and budget families under hash_variant = 1"""
    return [n for n in case_names() if META[n][0] in ("distance", "budget") and n not in NOT_UNDER_HASH_VARIANT_1]


def hash_variant_case(name):
    return case(name, _SEEDS_HASH_VARIANT_1[name]) if name in _SEEDS_HASH_VARIANT_1 else case(name)
