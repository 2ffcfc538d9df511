"""A small deflate READER for tests, the counterpart of tests/deflate_builder.py: a zlib stream as one record per block, with
everything an encoder decided in it -- block kinds and bit positions, the three code-length lists of a dynamic block and the
bit-length symbols as they were sent, the symbols with their sizes in bits, the histograms the trees were built from.  Pure
Python, no dependency on the library under test (RFC 1950 / 1951; tools/deflate_tokens.py is the same parse, symbol by symbol).

  blocks = read(z)
  blocks[0].kind, .final, .bit_pos, .bits            # "stored" / "fixed" / "dynamic"; the header's first bit; header to END_BLOCK
  blocks[0].hlit, .hdist, .hclen, .bl_lengths, .lit_lengths, .dist_lengths, .sent      # a dynamic block's header
  blocks[0].symbols, .sym_bits, .lit_hist, .dist_hist                                  # END_BLOCK is counted, and sized last
  replay(blocks)                                     # the plaintext

optimal_cost() and code_cost() say whether a length-limited code is still an optimal one (repair_ran); k9_max_pending()
restates the accumulator of the bit-packing kernel's per-thread loop (zs_kernels.hip, zs_emit_bits_kernel)."""
import heapq
import zlib

from deflate_builder import CL_ORDER, DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, MAX_BITS

END_BLOCK = 256
_FIXED_LIT_LENGTHS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_DIST_LENGTHS = [5] * 30  # (codes 30 and 31 of the fixed code never occur in a conformant stream)


class Block:
    """One block.  Fields that a kind does not have are None."""
    kind = final = bit_pos = bits = None
    len = data = None                                                    # stored
    hlit = hdist = hclen = bl_lengths = sent = None                      # dynamic
    lit_lengths = dist_lengths = None                                    # dynamic; the fixed code's for a fixed block
    symbols = sym_bits = lit_hist = dist_hist = None                     # fixed and dynamic

    def __repr__(self):
        return "Block(%s%s, bit %d, %d bits)" % (self.kind, ", final" if self.final else "", self.bit_pos, self.bits)


def _table(lengths):
    """Decoding table of a canonical code, indexed by the next `width` bits of the stream (LSB first): symbol << 4 | length, 0
    where no code begins.  An over-subscribed code raises; an incomplete one leaves holes."""
    width = max(lengths) if lengths else 0
    if width == 0:
        return [0], 0
    count = [0] * (MAX_BITS + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * (MAX_BITS + 2)
    for bits in range(1, MAX_BITS + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    if sum(count[l] << (MAX_BITS - l) for l in range(1, MAX_BITS + 1)) > 1 << MAX_BITS:
        raise ValueError("over-subscribed code")
    table = [0] * (1 << width)
    for s, l in enumerate(lengths):
        if l:
            c, r = nxt[l], 0
            nxt[l] += 1
            for _ in range(l):
                r = (r << 1) | (c & 1)
                c >>= 1
            table[r::1 << l] = [s << 4 | l] * (1 << (width - l))
    return table, (1 << width) - 1


_FIXED = (_table(_FIXED_LIT_LENGTHS), _table(_FIXED_DIST_LENGTHS))


class _Bits:
    """The stream as an accumulator of at least 48 valid bits, refilled eight bytes at a time; bytes past the end read as zero
    and are caught by the position check of read()."""

    def __init__(self, data, byte_pos):
        self.d, self.p, self.acc, self.n = data, byte_pos, 0, 0

    @property
    def pos(self):
        return self.p * 8 - self.n

    def peek(self, nbits):
        if self.n < nbits:
            self.acc |= int.from_bytes(self.d[self.p:self.p + 8], "little") << self.n
            self.p += 8
            self.n += 64
        return self.acc & ((1 << nbits) - 1)

    def get(self, nbits):
        v = self.peek(nbits)
        self.acc >>= nbits
        self.n -= nbits
        return v

    def seek(self, bit_pos):
        self.p, self.acc, self.n = bit_pos >> 3, 0, 0
        self.get(bit_pos & 7)


def _dynamic_header(b, blk):
    blk.hlit, blk.hdist, blk.hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
    if blk.hlit > 286 or blk.hdist > 30:
        raise ValueError("too many length or distance symbols")
    cl = [0] * 19
    for s in CL_ORDER[:blk.hclen]:
        cl[s] = b.get(3)
    blk.bl_lengths = cl
    table, mask = _table(cl)
    lens, sent = [], []
    while len(lens) < blk.hlit + blk.hdist:
        e = table[b.peek(7) & mask]
        if not e:
            raise ValueError("bad bit-length code")
        b.get(e & 15)
        s = e >> 4
        if s < 16:
            lens.append(s)
            sent.append((s, 1))
        elif s == 16:
            if not lens:
                raise ValueError("repeat with no length before it")
            r = 3 + b.get(2)
            lens += [lens[-1]] * r
            sent.append((16, r))
        else:
            r = 3 + b.get(3) if s == 17 else 11 + b.get(7)
            lens += [0] * r
            sent.append((s, r))
    if len(lens) > blk.hlit + blk.hdist:
        raise ValueError("a repeat runs past the last code length")
    blk.sent = sent
    blk.lit_lengths, blk.dist_lengths = lens[:blk.hlit], lens[blk.hlit:]
    if not blk.lit_lengths[END_BLOCK]:
        raise ValueError("no end-of-block code")
    return _table(blk.lit_lengths), _table(blk.dist_lengths)


def _symbols(b, blk, lit, dist):
    """The block's symbols up to END_BLOCK: a literal byte, or (length, distance)."""
    (lt, lmask), (dt, dmask) = lit, dist
    syms, sizes, lh, dh = [], [], [0] * 286, [0] * 30
    d, p, acc, n = b.d, b.p, b.acc, b.n  # (get() inlined: this loop is the reader's time)
    while True:
        if n < 48:
            acc |= int.from_bytes(d[p:p + 8], "little") << n
            p += 8
            n += 64
        e = lt[acc & lmask]
        l = e & 15
        s = e >> 4
        if not l:
            raise ValueError("bad literal / length code at bit %d" % (p * 8 - n))
        acc >>= l
        n -= l
        lh[s] += 1
        if s < 256:
            syms.append(s)
            sizes.append(l)
            continue
        if s == END_BLOCK:
            sizes.append(l)
            break
        c = s - 257
        if c > 28:
            raise ValueError("length symbol %d" % s)
        x = LEN_EXTRA[c]
        length = LEN_BASE[c] + (acc & ((1 << x) - 1))
        acc >>= x
        n -= x
        e = dt[acc & dmask]
        dl = e & 15
        dc = e >> 4
        if not dl or dc > 29:
            raise ValueError("bad distance code at bit %d" % (p * 8 - n))
        acc >>= dl
        n -= dl
        y = DIST_EXTRA[dc]
        syms.append((length, DIST_BASE[dc] + (acc & ((1 << y) - 1))))
        acc >>= y
        n -= y
        dh[dc] += 1
        sizes.append(l + x + dl + y)
    b.p, b.acc, b.n = p, acc, n
    blk.symbols, blk.sym_bits, blk.lit_hist, blk.dist_hist = syms, sizes, lh, dh


def read(z, raw=False):
    """The blocks of a zlib stream (raw: of a bare deflate stream).  Raises ValueError on a stream that is not conformant:
    header, codes, LEN / NLEN, a distance before the first byte, the Adler-32 trailer, bytes left over."""
    z = bytes(z)
    if not raw:
        if len(z) < 6 or (z[0] & 15) != 8 or (z[0] << 8 | z[1]) % 31 or z[1] & 32:
            raise ValueError("no zlib header")
    b = _Bits(z, 0 if raw else 2)
    blocks = []
    while True:
        blk = Block()
        blk.bit_pos = b.pos
        blk.final, typ = bool(b.get(1)), b.get(2)
        if typ == 0:
            blk.kind = "stored"
            b.seek((b.pos + 7) & ~7)
            blk.len, nlen = b.get(16), b.get(16)
            if blk.len ^ nlen != 0xFFFF:
                raise ValueError("LEN / NLEN")
            at = b.pos >> 3
            blk.data = z[at:at + blk.len]
            b.seek(b.pos + 8 * blk.len)
        elif typ == 1:
            blk.kind = "fixed"
            blk.lit_lengths, blk.dist_lengths = list(_FIXED_LIT_LENGTHS), list(_FIXED_DIST_LENGTHS)
            _symbols(b, blk, *_FIXED)
        elif typ == 2:
            blk.kind = "dynamic"
            _symbols(b, blk, *_dynamic_header(b, blk))
        else:
            raise ValueError("block type 3")
        blk.bits = b.pos - blk.bit_pos
        blocks.append(blk)
        if blk.final:
            break
    end = (b.pos + 7) >> 3
    if end + (0 if raw else 4) != len(z):
        raise ValueError("the stream ends at byte %d of %d" % (end, len(z)))
    if not raw and zlib.adler32(replay(blocks)) != int.from_bytes(z[end:], "big"):
        raise ValueError("Adler-32")
    return blocks


def replay(blocks):
    """The plaintext: every block's symbols applied."""
    out = bytearray()
    for blk in blocks:
        if blk.kind == "stored":
            out += blk.data
            continue
        for t in blk.symbols:
            if t.__class__ is int:
                out.append(t)
                continue
            length, d = t
            if d > len(out):
                raise ValueError("distance %d at byte %d" % (d, len(out)))
            if d >= length:
                out += out[len(out) - d:len(out) - d + length]
            else:
                out += (bytes(out[len(out) - d:]) * (length // d + 1))[:length]
    return bytes(out)


# ------------------------------------------------------------------ what the trees cost
def optimal_cost(freqs):
    """Bits an optimal prefix code spends on the symbols of this histogram, extra bits aside: the sum of the merged weights of
    Huffman's algorithm, whatever the ties.  One symbol in use costs a bit each time (a code has no 0-bit word)."""
    heap = [f for f in freqs if f > 0]
    if len(heap) < 2:
        return sum(heap)
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        f = heapq.heappop(heap) + heapq.heappop(heap)
        cost += f
        heapq.heappush(heap, f)
    return cost


def code_cost(freqs, lengths):
    if any(f and not l for f, l in zip(freqs, lengths)) or any(freqs[len(lengths):]):
        raise ValueError("a symbol in use has no code")
    return sum(f * l for f, l in zip(freqs, lengths))


def repair_ran(freqs, lengths, limit):
    """The encoder's overflow repair (Gen_bitlen's second half) changed this code: its longest word is the limit, and it costs
    more than an optimal code of its histogram.  (A code that reaches the limit without help costs the optimum.)"""
    return max(lengths) == limit and code_cost(freqs, lengths) > optimal_cost(freqs)


def bl_hist(block):
    """The histogram of a dynamic block's bit-length tree: the symbols sent."""
    h = [0] * 19
    for s, _ in block.sent:
        h[s] += 1
    return h


# ------------------------------------------------------------------ the bit-packing kernel's accumulator
def k9_max_pending(block):
    """zs_emit_bits_kernel, "---- pack": a thread takes 8 consecutive symbols, counted from the block's first (END_BLOCK is the
    last symbol), adds each to a 64-bit accumulator and, once that holds 16 bits or more, puts its whole bytes -- 56 bits at the
    most.  Returns the most bits the accumulator held at a put."""
    worst = 0
    for g in range(0, len(block.sym_bits), 8):
        fill = 0
        for nb in block.sym_bits[g:g + 8]:
            fill += nb
            if fill >= 16:
                worst = max(worst, fill)
                fill -= min(fill & ~7, 56)
    return worst
