"""A small deflate WRITER for tests: zlib streams built by hand, block by block, at the edges of the format that no encoder
visits (RFC 1950 / 1951).  Pure Python, no dependency on the library under test: the expected plaintext is kept by applying
every token that is written, and `zlib.decompress` / the oracle check the streams before the device sees them
(tests/test_deflate_builder.py).  One exception, data only: the catalogue's nested_english case takes its text from
zlibstream_amd.datagen (numpy, no native code), so catalogue() needs the repository root on sys.path; the Builder does not.

  b = Builder()
  b.dynamic_block([65, 66, (3, 2)], final=False)     # tokens: a literal byte, or (length, distance)
  b.stored_block(b"xyz", final=False, pad_ones=True)
  b.fixed_block([], final=True)
  z = b.finish()                                     # 78 9c, the blocks, Adler-32 of b.plaintext
  b.blocks                                           # [(kind, first bit, bits)] of every block; the first block is at bit 16

catalogue() returns the (name, stream, plaintext, expects_fallback) cases of tests/test_gpu_inflate_built.py; they are built
from fixed seeds at test time."""
import functools
import heapq
import random
import zlib

MAX_BITS = 15
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
PAR_MIN = 1024  # streams below it never reach the block-parallel pass

# length 3..258 -> (code - 257, extra value); 258 is code 285 (the alternative, 284 + 31, is dynamic_block's alt258)
_LEN_CODE = [None] * 259
for _c in range(28):
    for _e in range(1 << LEN_EXTRA[_c]):
        if LEN_BASE[_c] + _e < 258:
            _LEN_CODE[LEN_BASE[_c] + _e] = (_c, _e)
_LEN_CODE[258] = (28, 0)
_DIST_CODE = [None] * 32769
for _c in range(30):
    for _e in range(1 << DIST_EXTRA[_c]):
        _DIST_CODE[DIST_BASE[_c] + _e] = (_c, _e)


@functools.lru_cache(maxsize=None)
def _reverse(code, nbits):
    r = 0
    for _ in range(nbits):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical_codes(lengths):
    """The canonical Huffman codes (RFC 1951 3.2.2) of a list of code lengths: [(code, bits)], (0, 0) for an unused symbol.
    Lengths that are neither a complete code nor a single code of length 1 raise ValueError."""
    used = [l for l in lengths if l]
    if any(l < 0 or l > MAX_BITS for l in lengths) or not used:
        raise ValueError("code lengths out of range, or no code at all")
    kraft = sum(1 << (MAX_BITS - l) for l in used)
    if kraft != 1 << MAX_BITS and used != [1]:
        raise ValueError("neither a complete code nor one code of length 1 (Kraft sum %d / %d)" % (kraft, 1 << MAX_BITS))
    count = [0] * (MAX_BITS + 1)
    for l in used:
        count[l] += 1
    nxt, code = [0] * (MAX_BITS + 2), 0
    for bits in range(1, MAX_BITS + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        if l:
            out.append((nxt[l], l))
            nxt[l] += 1
        else:
            out.append((0, 0))
    return out


def huffman_lengths(freqs, limit):
    """Huffman code lengths of the symbols with freqs[s] > 0, none longer than `limit`: the frequencies are halved (never to
    zero) until the tree is shallow enough.  One symbol in use gets length 1."""
    freqs = list(freqs)
    live = [s for s, f in enumerate(freqs) if f > 0]
    lengths = [0] * len(freqs)
    if len(live) == 1:
        lengths[live[0]] = 1
        return lengths
    assert live and (1 << limit) >= len(live)
    while True:
        heap = [(freqs[s], s, (s,)) for s in live]
        heapq.heapify(heap)
        depth = dict.fromkeys(live, 0)
        while len(heap) > 1:
            fa, ta, a = heapq.heappop(heap)
            fb, tb, b = heapq.heappop(heap)
            for s in a + b:
                depth[s] += 1
            heapq.heappush(heap, (fa + fb, min(ta, tb), a + b))
        if max(depth.values()) <= limit:
            break
        for s in live:
            freqs[s] = (freqs[s] + 1) // 2
    for s in live:
        lengths[s] = depth[s]
    return lengths


def _rle_code_lengths(seq):
    """Code lengths as (symbol, extra value, extra bits) with the repeat codes 16 / 17 / 18."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, run = seq[i], 1
        while i + run < n and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11, 7))
                run -= r
            if run >= 3:
                out.append((17, run - 3, 3))
                run = 0
            out += [(0, 0, 0)] * run
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3, 2))
                run -= r
            out += [(v, 0, 0)] * run
    return out


_FIXED_LIT = canonical_codes([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_DIST = canonical_codes([5] * 32)


class Builder:
    def __init__(self):
        self.buf = bytearray(b"\x78\x9c")  # whole bytes written so far, the zlib header first: the first block is at bit 16
        self.acc, self.n = 0, 0  # the bits behind them, LSB first
        self.plaintext = bytearray()
        self.blocks = []         # (kind, first bit, bits)
        self.lengths = []        # per dynamic block, as written: (first bit, literal/length, distance, bit-length code lengths)

    # ---- bits
    @property
    def bit_pos(self):
        return len(self.buf) * 8 + self.n

    def put(self, value, nbits):
        """A field of nbits, least significant bit first."""
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        if self.n >= 64:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def code(self, code, nbits):
        """A Huffman code: most significant bit first."""
        self.put(_reverse(code, nbits), nbits)

    def align(self, ones=False):
        k = -self.n % 8
        self.put((1 << k) - 1 if ones else 0, k)

    def mark(self):
        return (len(self.buf), self.acc, self.n, len(self.plaintext), len(self.blocks), len(self.lengths))

    def rollback(self, m):
        """Forget everything written since mark() returned m (cases that are placed by a block's measured bit length)."""
        del self.buf[m[0]:]
        self.acc, self.n = m[1], m[2]
        del self.plaintext[m[3]:]
        del self.blocks[m[4]:]
        del self.lengths[m[5]:]

    # ---- blocks
    def _tokens(self, tokens, lit, dist, alt258):
        """tokens through the codes lit[sym] / dist[sym] = (code, bits); the plaintext follows."""
        lit = [(_reverse(c, l), l) if l else (0, 0) for c, l in lit]
        dist = [(_reverse(c, l), l) if l else (0, 0) for c, l in dist]
        out, buf, acc, n = self.plaintext, self.buf, self.acc, self.n  # (put() inlined: this loop is the builder's time)
        for t in tokens:
            if n >= 512:
                buf += (acc & ((1 << 512) - 1)).to_bytes(64, "little")
                acc >>= 512
                n -= 512
            if isinstance(t, int):
                c, l = lit[t]
                assert l, "literal %d has no code" % t
                acc |= c << n
                n += l
                out.append(t)
                continue
            length, d = t
            assert 3 <= length <= 258 and 1 <= d <= 32768 and d <= len(out), (t, len(out))
            lc, le = (27, 31) if alt258 and length == 258 else _LEN_CODE[length]
            c, l = lit[257 + lc]
            assert l, "length code %d has no code" % (257 + lc)
            acc |= (c | le << l) << n
            n += l + LEN_EXTRA[lc]
            dc, de = _DIST_CODE[d]
            c, l = dist[dc]
            assert l, "distance code %d has no code" % dc
            acc |= (c | de << l) << n
            n += l + DIST_EXTRA[dc]
            if d >= length:
                out += out[len(out) - d:len(out) - d + length]
            else:
                pat = bytes(out[len(out) - d:])
                out += (pat * (length // d + 1))[:length]
        self.acc, self.n = acc, n
        self.put(*lit[256])

    def dynamic_block(self, tokens, final, lit_lengths=None, dist_lengths=None, alt258=False):
        tokens = list(tokens)
        if lit_lengths is None or dist_lengths is None:
            lf, df = [0] * 286, [0] * 30
            lf[256] = 1
            for t in tokens:
                if isinstance(t, int):
                    lf[t] += 1
                else:
                    lf[257 + ((27 if alt258 and t[0] == 258 else _LEN_CODE[t[0]][0]))] += 1
                    df[_DIST_CODE[t[1]][0]] += 1
            if lit_lengths is None:
                lit_lengths = huffman_lengths(lf, MAX_BITS)
            if dist_lengths is None:
                dist_lengths = huffman_lengths(df, MAX_BITS) if any(df) else [0]
        lit_lengths, dist_lengths = list(lit_lengths), list(dist_lengths)
        assert len(lit_lengths) <= 286 and len(dist_lengths) <= 30 and len(lit_lengths) > 256 and lit_lengths[256]
        lit = canonical_codes(lit_lengths)
        # (no distance code at all: HDIST = 1 and a single zero length, for a block without matches)
        dist = canonical_codes(dist_lengths) if any(dist_lengths) else []
        hlit = max(257, max(i for i, l in enumerate(lit_lengths) if l) + 1)
        hdist = max([1] + [i + 1 for i, l in enumerate(dist_lengths) if l])
        # the lengths of both codes are one sequence for the repeat codes: a run may cross from one into the other
        seq = (lit_lengths + [0] * 286)[:hlit] + (dist_lengths + [0] * 30)[:hdist]
        rle = _rle_code_lengths(seq)
        cf = [0] * 19
        for s, _, _ in rle:
            cf[s] += 1
        if sum(1 for f in cf if f) == 1:  # one symbol alone is no complete code: a second one that is never written
            cf[0 if not cf[0] else 18] = 1
        cl = huffman_lengths(cf, 7)
        clc = canonical_codes(cl)
        hclen = max(4, max(i for i, s in enumerate(CL_ORDER) if cl[s]) + 1)
        start = self.bit_pos
        self.lengths.append((start, seq[:hlit], seq[hlit:], cl))
        self.put(1 if final else 0, 1), self.put(2, 2)
        self.put(hlit - 257, 5), self.put(hdist - 1, 5), self.put(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.put(cl[s], 3)
        for s, ev, eb in rle:
            self.code(*clc[s])
            self.put(ev, eb)
        self._tokens(tokens, lit, dist + [(0, 0)] * 30, alt258)
        self.blocks.append(("dynamic", start, self.bit_pos - start))
        return self.bit_pos - start

    def stored_block(self, data, final, pad_ones=False):
        data = bytes(data)
        assert len(data) <= 65535
        start = self.bit_pos
        self.put(1 if final else 0, 1), self.put(0, 2)
        self.align(pad_ones)
        self.put(len(data), 16), self.put(len(data) ^ 0xFFFF, 16)
        for i in range(0, len(data), 4096):
            self.put(int.from_bytes(data[i:i + 4096], "little"), 8 * len(data[i:i + 4096]))
        self.plaintext += data
        self.blocks.append(("stored", start, self.bit_pos - start))
        return self.bit_pos - start

    def fixed_block(self, tokens, final):
        start = self.bit_pos
        self.put(1 if final else 0, 1), self.put(1, 2)
        self._tokens(tokens, _FIXED_LIT, _FIXED_DIST, False)
        self.blocks.append(("fixed", start, self.bit_pos - start))
        return self.bit_pos - start

    def finish(self, pad_ones=False):
        self.align(pad_ones)
        assert self.n % 8 == 0
        body = bytes(self.buf) + self.acc.to_bytes(self.n // 8, "little")
        return body + zlib.adler32(bytes(self.plaintext)).to_bytes(4, "big")


LAYOUT = {}  # stream -> (its Builder's blocks, its Builder's lengths), for tests/test_deflate_reader.py


def _finish(b, pad_ones=False):
    z = b.finish(pad_ones)
    LAYOUT[z] = (tuple(b.blocks), tuple(b.lengths))
    return z, bytes(b.plaintext)


# ------------------------------------------------------------------ random complete codes and legal tokens (N; tools/fuzz_inflate.py)
def random_complete_lengths(rng, n):
    """n code lengths of a complete code, up to 15 bits: leaves of a complete code split at random."""
    if n == 1:
        return [1]
    leaves = [1, 1]
    while len(leaves) < n:
        can = [i for i, l in enumerate(leaves) if l < MAX_BITS]
        i = rng.choice(can)
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    return leaves


def random_block(b, rng, ntok, final):
    """One dynamic block with a random complete (not optimal) code over a random subset of the symbols, and random legal
    tokens of it."""
    lits = rng.sample(range(256), rng.randint(1, 256))
    lens = rng.sample(range(257, 286), rng.randint(0, 29))
    dists = sorted(rng.sample(range(30), rng.randint(1, 30))) if lens else []
    syms = lits + lens + [256]
    lit_lengths = [0] * 286
    for s, l in zip(syms, random_complete_lengths(rng, len(syms))):
        lit_lengths[s] = l
    dist_lengths = [0] * 30
    for s, l in zip(dists, random_complete_lengths(rng, len(dists)) if dists else []):
        dist_lengths[s] = l
    alt258 = 285 not in lens
    tokens, produced = [], len(b.plaintext)
    for _ in range(ntok):
        s = rng.choice(syms[:-1])
        if s >= 257:
            ok = [d for d in dists if DIST_BASE[d] <= produced]
            if not ok:
                s = rng.choice(lits)
            else:
                c = s - 257
                length = LEN_BASE[c] + rng.randrange(1 << LEN_EXTRA[c])
                if c == 27 and length == 258 and not alt258:
                    length = 257
                d = rng.choice(ok)
                dist = min(DIST_BASE[d] + rng.randrange(1 << DIST_EXTRA[d]), produced)
                tokens.append((length, dist))
                produced += length
                continue
        tokens.append(s)
        produced += 1
    b.dynamic_block(tokens, final, lit_lengths, dist_lengths, alt258)


def random_codes_stream(rng):
    """A stream of 1..12 such blocks, padded to the block-parallel minimum by a leading block of random literals."""
    nblocks = rng.randint(1, 12)
    sizes = [rng.choice([0, 1, 50, 300, 2000, 6000]) + rng.randrange(40) for _ in range(nblocks)]
    for pad in (0, 1200):
        b = Builder()
        if pad:
            b.dynamic_block(rng.randbytes(pad), False)
        for k, n in enumerate(sizes):
            random_block(b, rng, n, k == nblocks - 1)
        z, p = _finish(b, pad_ones=bool(rng.getrandbits(1)))
        if len(z) >= PAR_MIN:
            return z, p
    raise AssertionError("unreachable")


# ------------------------------------------------------------------ the catalogue
def _len_edges():
    # (code 284's largest extra value, 31, is length 258 again -- alt258's; its largest ordinary one is 30: length 257)
    return sorted({LEN_BASE[c] + e for c in range(29) for e in (0, (1 << LEN_EXTRA[c]) - 1)} | {257})


def _dist_edges():
    return sorted({DIST_BASE[c] + e for c in range(30) for e in (0, (1 << DIST_EXTRA[c]) - 1)})


def _all_codes():
    rng = random.Random(101)
    b = Builder()
    b.dynamic_block(rng.randbytes(40000), False)
    b.dynamic_block([(l, d) for l in _len_edges() for d in _dist_edges()], True)  # (258, 32768) among them
    return [("all_codes",) + _finish(b) + (False,)]


def _deep_codes():
    rng = random.Random(102)
    shape = list(range(1, 16)) + [15]
    lit_syms = [256, 285, 270, 101, 32, 257, 116, 97, 258, 111, 110, 264, 105, 0, 255, 115]  # end-of-block takes 15 bits
    lit_lengths = [0] * 286
    for s, l in zip(lit_syms, reversed(shape)):
        lit_lengths[s] = l
    dist_lengths = list(reversed(shape))  # distance symbols 0..15: distances 1..255
    b = Builder()
    tokens, produced = [], 0
    for _ in range(20000):
        s = rng.choice(lit_syms[1:])
        if s < 256 or produced < 256:
            tokens.append(s if s < 256 else 32)
            produced += 1
        else:
            c, d = s - 257, rng.randrange(16)
            tokens.append((LEN_BASE[c] + rng.randrange(1 << LEN_EXTRA[c]), DIST_BASE[d] + rng.randrange(1 << DIST_EXTRA[d])))
            produced += tokens[-1][0]
    used_l = {257 + _LEN_CODE[t[0]][0] if not isinstance(t, int) else t for t in tokens}
    used_d = {_DIST_CODE[t[1]][0] for t in tokens if not isinstance(t, int)}
    assert used_l == set(lit_syms[1:]) and used_d == set(range(16))  # the 14- and 15-bit symbols occur
    b.dynamic_block(tokens, True, lit_lengths, dist_lengths)
    return [("deep_codes",) + _finish(b) + (False,)]


def _c_cases():
    rng = random.Random(103)
    out = []
    b = Builder()
    b.dynamic_block(rng.randbytes(1200), False)
    b.dynamic_block([7] + [(258, 1)] * 40 + [(258, 300), 9, (258, 258), (258, 1200), (257, 2)], False, alt258=True)  # 258 = 284 + 31
    b.dynamic_block([(258, 1), 8, (258, 1), (258, 259)], True)                                                # 258 = 285, beside it
    out.append(("alt258",) + _finish(b) + (False,))
    b = Builder()
    b.dynamic_block(rng.randbytes(32768), False)
    b.dynamic_block([(258, 32768)] + [(258, 1)] * 300 + list(rng.randbytes(50)) + [(3, 32768), (258, 1), (4, 32767)] + [(258, 1)] * 130, True)
    out.append(("far_and_near",) + _finish(b) + (False,))
    b = Builder()
    b.dynamic_block(rng.randbytes(5000), False)
    b.dynamic_block([(258, 5000)] + list(rng.randbytes(700)) + [(100, 5958)], False)  # reaches output byte 0, twice
    b.dynamic_block([(258, 5), (258, 1), (3, 3)] + list(rng.randbytes(300)), True)    # the source starts in the block before
    out.append(("straddle",) + _finish(b) + (False,))
    return out


def _empty(b, kind, final=False):
    if kind == "dynamic":
        b.dynamic_block([], final)
    elif kind == "stored":
        b.stored_block(b"", final)
    else:
        b.fixed_block([], final)


def _empties():
    """Empty blocks of each kind as the first block (bit 16), between data blocks and as the final one, in runs of 1, 2 and 70.
    The large streams are above the sizes under which the walking chain kernel leaves a stream with unmeasured compressed
    blocks to the one-wave decoder (kWalkMinInput, and 48 KiB for fixed blocks); empties_small is below them."""
    out = []
    for name, kinds, data, fallback in (("empties_dynamic", ["dynamic"], 110000, False), ("empties_stored", ["stored"], 110000, False),
                                        ("empties_fixed", ["fixed"], 110000, False), ("empties_mixed", ["dynamic", "stored", "fixed"], 110000, False),
                                        ("empties_small", ["dynamic", "stored", "fixed"], 600, True)):
        rng = random.Random(104)
        b = Builder()
        k = 0
        for run in (1, 2, 70):
            for _ in range(run):
                _empty(b, kinds[k % len(kinds)])
                k += 1
            d = rng.randbytes(data)
            if run == 1:
                b.dynamic_block(d, False)
            elif run == 2:
                for o in range(0, len(d), 65535):
                    b.stored_block(d[o:o + 65535], False)
            else:
                b.fixed_block(list(d[:len(d) // 2]) + [(258, 1), (3, min(len(d) // 2, 32768))], False)
                b.dynamic_block(list(d[len(d) // 2:]) + [(258, 1), (3, min(len(d) // 2, 32768))], False)
        _empty(b, kinds[k % len(kinds)], True)
        out.append((name,) + _finish(b) + (fallback,))
    return out


def _nested():
    from zlibstream_amd import datagen  # (data only: the generator of the benchmark's text)
    rng = random.Random(105)
    out = []
    for name, inner in (("nested_letters", zlib.compress(bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz ") for _ in range(30000)))),
                        ("nested_english", zlib.compress(datagen.english(1 << 20, 7)))):
        b = Builder()
        for o in range(0, len(inner), 65535):
            b.stored_block(inner[o:o + 65535], False)
        n = len(inner)
        far = min(n, 32768)
        b.dynamic_block([(258, far), (200, far), 1, 2, (3, 2), (258, min(n, 700))] + list(rng.randbytes(1200)) + [(17, far)], True)
        out.append((name,) + _finish(b) + (False,))
    return out


def _stored_edges():
    rng = random.Random(106)
    b = Builder()
    b.dynamic_block(rng.randbytes(1200), False)
    for n in (0, 1, 65535, 0):
        b.stored_block(rng.randbytes(n), False, pad_ones=True)
    for want in range(8):  # the stored block's three header bits at every bit alignment, ones up to the byte's end
        m = b.mark()
        b.dynamic_block([65] * 9, False)
        k = 9 + (want - b.bit_pos) % 8  # 'A' and end-of-block are 1 bit each: a literal more is a bit more
        b.rollback(m)
        b.dynamic_block([65] * k, False)
        assert b.bit_pos % 8 == want
        b.stored_block(rng.randbytes(want + 1), False, pad_ones=True)
    for k in range(12, 20):  # ... and padding bits behind the final end-of-block
        m = b.mark()
        b.dynamic_block([65] * k + [(5, 3)], True)
        if b.bit_pos % 8:
            break
        b.rollback(m)
    assert b.bit_pos % 8
    return [("stored_edges",) + _finish(b, pad_ones=True) + (False,)]


def _tiny_blocks():
    rng = random.Random(107)
    out = []
    b = Builder()
    for i in range(4000):
        b.dynamic_block([rng.randrange(256), rng.randrange(256), (3, 2)], i == 3999)
    # more blocks than in_len / 96 + 64: zs_inflate_par.hip, max_blk
    out.append(("tiny_blocks_dense",) + _finish(b) + (True,))
    b = Builder()
    for i in range(300):
        b.dynamic_block(list(rng.randbytes(80)) + [(4, 30)], i == 299)
    z, p = _finish(b)
    # more than kFindMaxCand = 32 headers to a 4 KiB chunk of the finder overflow the chunk's list (zs_inflate_par.hip,
    # zs_inf_flatten_kernel: "a chunk's list overflowed"; DESIGN.md section 8, blocks of ~100 symbols) and the stream is handed
    # on: these blocks are about 120 bytes, 34 to a chunk
    assert 116 * 300 <= len(z) <= 124 * 300, len(z)
    out.append(("tiny_blocks_sparse", z, p, True))
    b = Builder()
    for i in range(300):
        b.dynamic_block(list(rng.randbytes(130)) + [(4, 30)], i == 299)  # 180 bytes a block, 23 to a chunk: the block-parallel pass's
    out.append(("small_blocks",) + _finish(b) + (False,))
    b = Builder()
    b.stored_block(b"abc", False)
    for i in range(20000):
        b.fixed_block([], i == 19999)
    out.append(("empty_fixed_run",) + _finish(b) + (True,))
    return out


def _fixed_all():
    out = []
    for name, n, fallback in (("fixed_all_large", 60000, False), ("fixed_all_small", 33000, True)):
        rng = random.Random(108)
        b = Builder()
        b.fixed_block(list(range(256)) + list(rng.randbytes(n - 256)), False)
        b.fixed_block([(l, d) for l in _len_edges() for d in _dist_edges() if (l + d) % 3 == 0 or l in (3, 258) or d in (1, 32768)], False)
        b.fixed_block(list(range(255, -1, -1)) + [(258, 1), (3, 32768)], True)
        z, p = _finish(b)
        assert (len(z) > 48 * 1024) == (not fallback)  # fixed blocks below 48 KiB are the one-wave decoder's
        out.append((name, z, p, fallback))
    return out


def _long_blocks():
    out = []
    for name, n, fallback in (("long_block_under", 600000, False), ("long_block_over", 1200000, True)):  # kParMaxSyms = 1 << 20
        b = Builder()
        b.dynamic_block(random.Random(109).randbytes(n), True)
        out.append((name,) + _finish(b) + (fallback,))
    return out


def _dependent_chain():
    b = Builder()
    b.dynamic_block([1, 2, 3] + [(3, 3)] * 5000 + [(4, 3)] * 3000 + [(258, 2)] * 100 + [(3, 1)] * 2000, True)
    return [("dependent_chain",) + _finish(b) + (False,)]


def _tile_edges():
    rng = random.Random(111)
    b = Builder()
    for p in range(4090, 4101):  # an edge of a 4096-cell step inside the match at every offset
        b.dynamic_block(list(rng.randbytes(p)) + [(258, 1)] + list(rng.randbytes(5000)), False)
    b.dynamic_block([(258, 1)] * 20, False)      # the step is cut by cells
    # (literals are a cell a token: the blocks above are cut by tokens long before 4096 cells.  These are cut by cells, the 16th
    # match across the edge at every offset, its cells exactly up to the edge at q = 226, and the next step's first cells copy
    # out of the ring behind them; 200 literals behind keep the blocks above 128 bytes, see tiny_blocks_sparse)
    for q in range(259):
        b.dynamic_block(list(rng.randbytes(q)) + [(258, 1)] * 15 + [(258, 258), (258, 4096), (5, 4095), (258, 1)] + list(rng.randbytes(200)), False)
    b.dynamic_block(rng.randbytes(3000), True)   # the step is cut by tokens
    return [("tile_edges",) + _finish(b) + (False,)]


def _subsequence_edges():
    """Blocks of a flat literal code (0..254: 8 bits; 255 and end-of-block: 9) whose length in bits, header included, is one
    below, exactly and one above 1024 and 65536: 9-bit literals set the length to the bit."""
    rng = random.Random(112)
    flat = [8] * 255 + [9, 9]
    b = Builder()
    b.dynamic_block(rng.randbytes(1200), False)
    for target in (1024, 65536):
        for want in (target - 1, target, target + 1):
            m = b.mark()
            empty = b.dynamic_block([], False, flat, [0])
            b.rollback(m)
            nine = (want - empty) % 8
            eight = (want - empty - 9 * nine) // 8
            toks = [rng.randrange(255) for _ in range(eight)]
            for _ in range(nine):
                toks.insert(rng.randrange(len(toks) + 1), 255)
            assert b.dynamic_block(toks, False, flat, [0]) == want
    b.dynamic_block([(258, 1)], True)
    return [("subsequence_edges",) + _finish(b) + (False,)]


def _marker_limit():
    """The lane decoder (blocks with checkpoints and no tokens; every measured block under ZS_INF_MEASURE_DBG=3) writes a source
    before its sub-block as a marker, "d cells before the sub-block's first", d <= 32512 (kSubMarkMax, zs_inflate_par.hip); a
    source further back inside the block fails the stream over.  Here matches sit exactly on the limit.  Every symbol of the
    block is a multiple of 8 bits (literals 8; a match 9 + 2 + 13), so the sub-blocks -- 64 subsequences of S bits from the
    block's first symbol, S = the stream's bits / 64 rounded up to a multiple of 64 -- begin at symbols the builder knows: the
    first symbol of a sub-block is (258, 32512), or a literal and then (258, 32513)."""
    lit_lengths = [8] * 254 + [9, 9, 9] + [0] * 28 + [9]   # 0..253; 254, 255, end-of-block, 285
    dist_lengths = [1, 2] + [0] * 27 + [2]                  # distance codes 0, 1 and 29 (24577..32768: 13 extra bits)
    slots, sub = 40704, 5120                                # symbols of 8 bits in the block; the subsequence length this gives
    per = sub // 8
    out = []
    # marker_limit_over: the same stream but for one match that is one cell beyond the limit -- handed on when the block is the
    # lane decoder's (NO_TOKENS_FALLBACK), the expand kernel's otherwise
    for name, over in (("marker_limit", 0), ("marker_limit_over", 1)):
        rng = random.Random(114)
        toks, produced, k = [], 0, 0
        for j in range(0, slots, per):
            n = min(per, slots - j)
            if produced >= 32512 + 1 and n == per:          # a sub-block that begins more than 32512 bytes into the block
                lead = k % 2
                toks += [rng.randrange(254) for _ in range(lead)] + [(258, 32512 + lead + (over if k == 5 else 0))]
                produced += lead + 258
                n -= lead + 3
                k += 1
            toks += [rng.randrange(254) for _ in range(n)]
            produced += n
        assert k >= 8
        b = Builder()
        b.dynamic_block(toks, True, lit_lengths, dist_lengths)
        z, p = _finish(b)
        span = len(z) * 8 - 16
        assert ((span + 63) // 64 + 63) // 64 * 64 == sub, span  # (tok_sub_bits of zs_inflate_tok.hip for a block that ends the stream)
        out.append((name, z, p, False))
    return out


def _threshold():
    out = []
    for total in (PAR_MIN - 1, PAR_MIN, PAR_MIN + 1):
        rng = random.Random(113)
        b = Builder()
        b.dynamic_block(list(rng.randbytes(500)) + [(258, 1), (30, 400)], False)
        n = total - 4 - ((b.bit_pos + 3 + 7) // 8 + 4)  # the stored block's LEN / NLEN start at the next byte behind its header
        b.stored_block(rng.randbytes(n), True)
        z, p = _finish(b)
        assert len(z) == total
        # (the 1023-byte stream goes to the one-wave decoder below the minimum and is not counted)
        out.append(("threshold_%d" % total, z, p, False))
    return out


def _random_codes():
    out = []
    for seed in (1, 2):
        rng = random.Random(seed)
        for i in range(12):
            out.append(("random_codes_%d_%02d" % (seed, i),) + random_codes_stream(rng) + (False,))
    return out


# ZS_INF_MEASURE_DBG=3 (no tokens: every measured block is the lane decoder's) hands on what the default does, and all_codes:
# its second block is 200 KB of output with distances up to 32768, sources inside the block further before a sub-block than a
# marker can say (kSubMarkMax = 32512, zs_inflate_par.hip zs_inf_decode_lane_kernel; marker_limit sits exactly on that limit)
NO_TOKENS_FALLBACK = ("all_codes", "marker_limit_over")
MAX_STREAM = 1300000
MAX_TOTAL = 8 << 20


@functools.lru_cache(maxsize=None)
def catalogue():
    """[(name, stream, plaintext, expects_fallback)]: expects_fallback says whether the block-parallel pass hands the stream to
    the one-wave decoder (zs_ctx_counter "inf_wave_streams"); every True names its rule where the case is built."""
    cases = (_all_codes() + _deep_codes() + _c_cases() + _empties() + _nested() + _stored_edges() + _tiny_blocks() + _fixed_all() +
             _long_blocks() + _dependent_chain() + _tile_edges() + _subsequence_edges() + _marker_limit() + _threshold() + _random_codes())
    assert len({c[0] for c in cases}) == len(cases)
    assert all(len(c[1]) <= MAX_STREAM for c in cases) and sum(len(c[1]) for c in cases) <= MAX_TOTAL
    return tuple(cases)


def case_names():
    """The catalogue's names without building it (for parametrised tests)."""
    return (["all_codes", "deep_codes", "alt258", "far_and_near", "straddle", "empties_dynamic", "empties_stored", "empties_fixed",
             "empties_mixed", "empties_small", "nested_letters", "nested_english", "stored_edges", "tiny_blocks_dense", "tiny_blocks_sparse", "small_blocks",
             "empty_fixed_run", "fixed_all_large", "fixed_all_small", "long_block_under", "long_block_over", "dependent_chain",
             "tile_edges", "subsequence_edges", "marker_limit", "marker_limit_over"] + ["threshold_%d" % n for n in (1023, 1024, 1025)] +
            ["random_codes_%d_%02d" % (s, i) for s in (1, 2) for i in range(12)])


def case(name):
    return next(c for c in catalogue() if c[0] == name)
