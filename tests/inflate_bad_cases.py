"""Malformed zlib streams, one per rule of RFC 1950 / 1951 that inflate enforces, each beside the nearest legal stream: the
catalogue of tests/test_inflate_bad_cases.py (every claim against the oracle and zlib, on the CPU) and of
tests/test_gpu_inflate_bad_cases.py (the device gives the same code, message, length and bytes).  Streams are written bit by
bit with deflate_builder.Builder from fixed seeds at import time; nothing here touches the library under test.

A case is (name, stream, rc, message, out_len, plaintext_prefix):
  rejected      rc / message are the claim, out_len the bytes produced before the refusal, plaintext_prefix those bytes;
  accepted twin rc is ZS_STREAM_END, message None, plaintext_prefix the whole plaintext.
capacity(case) is the output room every test gives the case: the plaintext for a twin, 300 bytes more than the prefix for a
rejected stream (room for the refused token, so that the rule and not the room is what fires).

META[name] = (rule, side, placement); RULES[rule] = {"rejected": [names], "accepted": [names]} (a legal stream may stand on the
accepted side of several rules: the one good header is the twin of every header rule).

Placements of a rejected case (header cases cannot be placed: they get a short and a long body, and only the header decides):
  first        the bad block is the stream's first, the stream below 1 KiB: the one-wave decoder directly;
  behind_6k    behind three non-final dynamic blocks of 2 000 random literals: the block-parallel pass takes the stream,
               and has to hand it on;
  behind_100k  behind more than 100 000 bytes of matches and literals: beyond the one-wave decoder's 64 KiB ring and two of
               its flushes, so the length at the refusal counts bytes that are still in the ring.

One rule has no legal twin.  A bit-length code of a single 1-bit code is accepted by the rule (Huft_build's exception), but
no legal block can follow: with one symbol v in use, all HLIT + HDIST >= 258 code lengths are v (or all zero, v = 17 / 18), and
257 or more literal/length codes of one length are never a complete code nor a single code.  Its accepted side holds streams
that pass the rule and are refused by a later one (PASSES_ONLY): the message of the later rule is the evidence.

sweep() is one legal stream of every block kind; the tests cut it at every length (cuts) and give it every short capacity
(caps)."""
import functools
import random

import deflate_builder as db
from deflate_builder import Builder

ZS_STREAM_END, ZS_NEED_DICT, ZS_DATA_ERROR, ZS_BUF_ERROR = 1, 2, -3, -5
PLACEMENTS = ("first", "behind_6k", "behind_100k")
SLACK = 300  # output room behind a rejected stream's prefix: more than the longest refused token (258)

FLAT = [8] * 255 + [9, 9]            # literals 0..254: 8 bits; 255 and end-of-block: 9.  Complete, HLIT = 257
WITH_LEN = [8] * 254 + [9] * 4       # 0..253: 8 bits; 254, 255, end-of-block and length code 257 (length 3): 9.  HLIT = 258
DIST_TEN = [9, 9, 8, 7, 6, 5, 4, 3, 2, 1]  # a complete distance code that begins with the literal code's last length


def _clone(b):
    c = Builder()
    c.buf, c.acc, c.n = bytearray(b.buf), b.acc, b.n
    c.plaintext, c.blocks, c.lengths = bytearray(b.plaintext), list(b.blocks), list(b.lengths)
    return c


@functools.lru_cache(maxsize=None)
def _prefix_builder(placement):
    b = Builder()
    if placement == "behind_6k":
        rng = random.Random(201)
        for _ in range(3):
            b.dynamic_block(rng.randbytes(2000), False)
    elif placement == "behind_100k":
        rng = random.Random(202)
        produced = 0
        for k in range(3):
            toks = list(rng.randbytes(1500))
            produced += 1500
            while produced < (k + 1) * 34000:
                if rng.random() < 0.3:
                    toks.append(rng.randrange(256))
                    produced += 1
                else:
                    length = rng.choice((3, 4, 17, 100, 258, 258))
                    toks.append((length, min(rng.choice((1, 2, 300, 5000, 32768, produced)), produced, 32768)))
                    produced += length
            b.dynamic_block(toks, False)
        assert len(b.plaintext) >= 100000
    else:
        assert placement == "first"
    return b


def _prefix(placement):
    return _clone(_prefix_builder(placement))


def _codes(lengths):
    """canonical_codes without its refusal: the codes a decoder assigns to an incomplete code (never used for an
    oversubscribed one, which no decoder gets past)."""
    count = [0] * (db.MAX_BITS + 2)
    for l in lengths:
        if l:
            count[l] += 1
    nxt, code = [0] * (db.MAX_BITS + 2), 0
    for bits in range(1, db.MAX_BITS + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        out.append((nxt[l], l) if l else (0, 0))
        nxt[l] += 1 if l else 0
    return out


def _sym(b, codes, s):
    c, l = codes[s]
    assert l, "symbol %d has no code" % s
    b.code(c, l)


def _dyn_header(b, final, lit_lengths, dist_lengths, rle=None, cl=None):
    """A dynamic block's header, unchecked: HLIT / HDIST are the lists' lengths, `rle` the code-length sequence as
    (symbol, extra value, extra bits) -- the builder's own by default --, `cl` the 19 bit-length code lengths -- a Huffman
    code of the sequence's symbols by default.  All 19 are written.  Returns the codes of both trees."""
    lit_lengths, dist_lengths = list(lit_lengths), list(dist_lengths)
    if rle is None:
        rle = db._rle_code_lengths(lit_lengths + dist_lengths)
    if cl is None:
        cf = [0] * 19
        for s, _, _ in rle:
            cf[s] += 1
        if sum(1 for f in cf if f) == 1:
            cf[0 if not cf[0] else 18] = 1
        cl = db.huffman_lengths(cf, 7)
    clc = _codes(cl)
    b.put(1 if final else 0, 1), b.put(2, 2)
    b.put(len(lit_lengths) - 257, 5), b.put(len(dist_lengths) - 1, 5), b.put(15, 4)
    for s in db.CL_ORDER:
        b.put(cl[s], 3)
    for s, ev, eb in rle:
        _sym(b, clc, s)
        b.put(ev, eb)
    return _codes(lit_lengths), _codes(dist_lengths)


def _emit(b, tokens, lit, dist):
    """Tokens through the given codes, the plaintext kept; a match that reaches before the first byte is written and ends
    the emission (False): a decoder refuses it there."""
    for t in tokens:
        if isinstance(t, int):
            _sym(b, lit, t)
            b.plaintext.append(t)
            continue
        length, d = t
        lc, le = db._LEN_CODE[length]
        _sym(b, lit, 257 + lc)
        b.put(le, db.LEN_EXTRA[lc])
        dc, de = db._DIST_CODE[d]
        _sym(b, dist, dc)
        b.put(de, db.DIST_EXTRA[dc])
        if d > len(b.plaintext):
            return False
        for _ in range(length):
            b.plaintext.append(b.plaintext[-d])
    return True


def _raw_block(b, tokens, final):
    """A dynamic block with the Huffman codes of its tokens, like Builder.dynamic_block, but unchecked: a match may reach
    too far (the block then ends at that match)."""
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        else:
            lf[257 + db._LEN_CODE[t[0]][0]] += 1
            df[db._DIST_CODE[t[1]][0]] += 1
    ll = db.huffman_lengths(lf, db.MAX_BITS)
    dl = db.huffman_lengths(df, db.MAX_BITS)
    ll = ll[:max(257, max(i for i, l in enumerate(ll) if l) + 1)]
    dl = dl[:max(i for i, l in enumerate(dl) if l) + 1]
    lit, dist = _dyn_header(b, final, ll, dl)
    if _emit(b, tokens, lit, dist):
        _sym(b, lit, 256)


def _filler(b):
    """Bits behind a refusal: a decoder that reads a code nobody has goes on to its 15th bit before it gives up, and must find
    the bits (a stream that ends inside them is a truncated one, another class)."""
    b.put(0x5A5A5A5A5A, 40)


# ------------------------------------------------------------------ the catalogue's bookkeeping
_CASES, META, RULES = [], {}, {}
PASSES_ONLY = {}  # name -> the rule it passes although a later one refuses it (see the module's text)


def _add(name, z, rc, message, prefix, rule, side, placement, also=()):
    assert name not in META, name
    prefix = bytes(prefix)
    _CASES.append((name, bytes(z), rc, message, len(prefix), prefix))
    META[name] = (rule, side, placement)
    for r in (rule,) + tuple(also):
        RULES.setdefault(r, {"rejected": [], "accepted": []})[side].append(name)


def _rejected(base, rule, message, writer, rc=ZS_DATA_ERROR, placements=PLACEMENTS, side="rejected", passes=None):
    for pl in placements:
        b = _prefix(pl)
        writer(b)
        _filler(b)
        z = b.finish()
        assert (len(z) < db.PAR_MIN) == (pl == "first"), (base, pl, len(z))
        name = "%s_%s" % (base, pl)
        _add(name, z, rc, message, b.plaintext, passes or rule, side, pl)
        if passes:
            PASSES_ONLY[name] = passes


def _twin(name, rule, b, placement="first", also=()):
    z = b.finish()
    _add(name, z, ZS_STREAM_END, None, b.plaintext, rule, "accepted", placement, also)


# ------------------------------------------------------------------ RFC 1950: the header
def _fcheck(cmf, flg):
    return flg + (31 - ((cmf << 8) + flg) % 31) % 31


def _header_cases():
    bodies = {}
    b = Builder()
    b.fixed_block(list(b"a short body ") + [(5, 3), (9, 13)], True)
    bodies["short"] = (b.finish(), bytes(b.plaintext))
    b = _prefix("behind_6k")
    b.dynamic_block(list(b"the long body's last block") + [(258, 26), (7, 200)], True)
    bodies["long"] = (b.finish(), bytes(b.plaintext))
    assert len(bodies["short"][0]) < db.PAR_MIN <= len(bodies["long"][0])
    for body, (z, plain) in bodies.items():
        for base, rule, hdr, rc, message in (
                ("cm_9", "CM", bytes([0x79, _fcheck(0x79, 0x80)]), ZS_DATA_ERROR, "unknown compression method"),
                ("cm_0", "CM", bytes([0x70, _fcheck(0x70, 0x80)]), ZS_DATA_ERROR, "unknown compression method"),
                # FCHECK made valid, so that the check behind the window size is not what fires
                ("cinfo_8", "CINFO", bytes([0x88, _fcheck(0x88, 0x80)]), ZS_DATA_ERROR, "invalid window size"),
                ("cinfo_15", "CINFO", bytes([0xF8, _fcheck(0xF8, 0x80)]), ZS_DATA_ERROR, "invalid window size"),
                ("fcheck_plus_1", "FCHECK", b"\x78\x9d", ZS_DATA_ERROR, "incorrect header check"),
                ("fcheck_zero", "FCHECK", b"\x78\x80", ZS_DATA_ERROR, "incorrect header check"),
                ("fdict", "FDICT", b"\x78\xbb", ZS_NEED_DICT, "need dictionary")):
            assert ((hdr[0] << 8) + hdr[1]) % 31 == 0 or rule == "FCHECK"
            _add("%s_%s" % (base, body), hdr + z[2:], rc, message, b"", rule, "rejected", body)
        _add("header_789c_%s" % body, z, ZS_STREAM_END, None, plain, "CINFO", "accepted", body, also=("CM", "FCHECK", "FDICT"))
    # a 256-byte window declared (CINFO 0); the short body's distances are below 256
    z, plain = bodies["short"]
    _add("cinfo_0_short", bytes([0x08, _fcheck(0x08, 0x00)]) + z[2:], ZS_STREAM_END, None, plain, "CINFO", "accepted", "short")


# ------------------------------------------------------------------ RFC 1951: block headers
def _block_header_cases():
    def btype3(final):
        return lambda b: (b.put(final, 1), b.put(3, 2))
    _rejected("btype_3_final", "BTYPE", "invalid block type", btype3(1))
    _rejected("btype_3", "BTYPE", "invalid block type", btype3(0), placements=("first", "behind_6k"))
    for pl in PLACEMENTS:  # the nearest legal stream: BTYPE 1 there, an empty fixed block
        b = _prefix(pl)
        b.fixed_block([], True)
        _twin("btype_1_%s" % pl, "BTYPE", b, pl)

    def stored(length, flip):
        def w(b):
            b.put(0, 1), b.put(0, 2)
            b.align()
            b.put(length, 16), b.put((length ^ 0xFFFF) ^ flip, 16)
            b.put(int.from_bytes(b"stored bytes"[:length], "little"), 8 * min(length, 12))
        return w
    _rejected("nlen_bit_8", "stored LEN/NLEN", "invalid stored block lengths", stored(12, 0x0100))
    _rejected("nlen_bit_0_len_0", "stored LEN/NLEN", "invalid stored block lengths", stored(0, 0x0001), placements=("first", "behind_6k"))
    _rejected("nlen_bit_15", "stored LEN/NLEN", "invalid stored block lengths", stored(12, 0x8000), placements=("first",))
    rng = random.Random(203)
    for name, n in (("stored_len_0", 0), ("stored_len_65535", 65535)):
        b = Builder()
        b.stored_block(rng.randbytes(n), False)
        b.stored_block(b"", True)
        _twin(name, "stored LEN/NLEN", b)

    def counts(hlit5, hdist5):
        return lambda b: (b.put(1, 1), b.put(2, 2), b.put(hlit5, 5), b.put(hdist5, 5), b.put(15, 4))
    _rejected("hlit_287", "HLIT / HDIST", "too many length or distance symbols", counts(30, 0))
    _rejected("hlit_288", "HLIT / HDIST", "too many length or distance symbols", counts(31, 0))
    _rejected("hdist_31", "HLIT / HDIST", "too many length or distance symbols", counts(0, 30))
    _rejected("hdist_32", "HLIT / HDIST", "too many length or distance symbols", counts(0, 31))
    # HLIT 286 and HDIST 30, both codes complete: 226 / 256 + 60 / 512 and 2 / 16 + 28 / 32
    b = _prefix("behind_100k")
    b.dynamic_block([0, 225, 226, 255, (258, 24577), (227, 32768), (3, 1)], True, [8] * 226 + [9] * 60, [4] * 2 + [5] * 28)
    assert len(b.lengths[-1][1]) == 286 and len(b.lengths[-1][2]) == 30
    _twin("hlit_286_hdist_30", "HLIT / HDIST", b, "behind_100k")


# ------------------------------------------------------------------ the bit-length code and the code-length sequence
def _bl_raw(cl, bits):
    """A dynamic header with HLIT 257, HDIST 1 and the given bit-length code lengths, then raw bits."""
    def w(b):
        b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(0, 5), b.put(15, 4)
        for s in db.CL_ORDER:
            b.put(cl[s], 3)
        for v, n in bits:
            b.put(v, n)
    return w


def _one(sym, length):
    return [length if s == sym else 0 for s in range(19)]


def _bit_length_cases():
    rule = "bit-length code"
    _rejected("bl_all_1", rule, "oversubscribed dynamic bit lengths tree", _bl_raw([1] * 19, []))
    _rejected("bl_three_of_1", rule, "oversubscribed dynamic bit lengths tree", _bl_raw([1, 1, 1] + [0] * 16, []), placements=("first",))
    _rejected("bl_one_of_2", rule, "incomplete dynamic bit lengths tree", _bl_raw(_one(8, 2), []))
    _rejected("bl_two_of_2", rule, "incomplete dynamic bit lengths tree", _bl_raw([2, 0, 0, 2] + [0] * 15, []), placements=("first",))
    # one code of length 1 alone passes (Huft_build's exception): 258 times the symbol 9 -- 257 literal/length codes of 9 bits
    _rejected("bl_one_of_1", "literal/length code", "incomplete literal/length tree", _bl_raw(_one(9, 1), [(0, 64)] * 4 + [(0, 2)]),
              side="accepted", passes=rule)
    # ... and its other code, the one no symbol has, is refused where it is read
    _rejected("bl_unused_code", "repeat", "invalid bit length repeat", _bl_raw(_one(8, 1), [(0, 3), (0xFFFFF, 20)]))
    PASSES_ONLY.update({"bl_unused_code_%s" % pl: rule for pl in PLACEMENTS})
    for pl in PLACEMENTS:
        RULES[rule]["accepted"].append("bl_unused_code_%s" % pl)


def _seq_block(b, lit_lengths, dist_lengths, rle, tokens, final=True):
    start = b.bit_pos
    lit, dist = _dyn_header(b, final, lit_lengths, dist_lengths, rle)
    ok = _emit(b, tokens, lit, dist)
    assert ok
    _sym(b, lit, 256)
    b.blocks.append(("dynamic", start, b.bit_pos - start))


def _repeat_cases():
    rule = "repeat"
    text = list(b"code lengths by repeat codes")
    flat_rle = db._rle_code_lengths(FLAT + [0])
    assert flat_rle[0][0] == 8 and flat_rle[1][0] == 16
    _rejected("rep_16_first", rule, "invalid bit length repeat", lambda b: _dyn_header(b, True, FLAT, [0], [(16, 0, 2)] + flat_rle))
    b = Builder()
    _seq_block(b, FLAT, [0], flat_rle, text)
    _twin("rep_16_second", rule, b)
    # a run that ends exactly at HLIT + HDIST, and one past it: the sequence's head by the builder, its last run by hand
    for sym, dist_lengths, head_extra, exact, ebits in ((16, [1, 3, 3, 3, 3], [1, 3], 3, 2), (17, [0] * 3, [], 3, 3), (18, [0] * 11, [], 11, 7),
                                                       (16, [1, 2] + [5] * 8, [1, 2, 5, 5], 6, 2), (17, [0] * 10, [], 10, 3), (18, [0] * 30, [], 30, 7)):
        head = db._rle_code_lengths(FLAT + head_extra)
        base = 11 if sym == 18 else 3
        tag = "rep_%d_run_%d" % (sym, exact)
        if exact + 1 - base < (1 << ebits):  # (the longest run of a 16 or 17 has no "one past": 6 and 10 are their limits)
            _rejected(tag + "_past_end", rule, "invalid bit length repeat",
                      lambda b, h=head, s=sym, e=exact, bs=base, eb=ebits, dl=dist_lengths: _dyn_header(b, True, FLAT, dl, h + [(s, e + 1 - bs, eb)]),
                      placements=PLACEMENTS if exact in (3, 11) else ("first",))
        b = Builder()
        _seq_block(b, FLAT, dist_lengths, head + [(sym, exact - base, ebits)], text)
        _twin(tag + "_to_end", rule, b)
    # one run from the literal lengths into the distance lengths: 9 (255), then a 16 over end-of-block and two distance codes
    rle = db._rle_code_lengths(FLAT + DIST_TEN)
    at, crossing = 0, []
    for s, ev, _ in rle:
        n = 1 if s < 16 else ev + (11 if s == 18 else 3)
        if at < 257 < at + n:
            crossing.append(s)
        at += n
    assert crossing == [16] and at == 267
    for pl in PLACEMENTS:
        b = _prefix(pl)
        _seq_block(b, FLAT, DIST_TEN, rle, text)
        _twin("rep_16_crosses_%s" % pl, rule, b, pl)
    # ... and zeros: lengths 257..259 unused, distance codes 0..2 unused, one 17 over all six
    rle = db._rle_code_lengths(FLAT) + [(17, 3, 3), (1, 0, 0)]
    b = Builder()
    _seq_block(b, FLAT + [0, 0, 0], [0, 0, 0, 1], rle, text)
    _twin("rep_17_crosses", rule, b)


# ------------------------------------------------------------------ the two trees
def _tree_cases():
    lit_rule, dist_rule = "literal/length code", "distance code"
    _rejected("lit_257_of_8", lit_rule, "oversubscribed literal/length tree", lambda b: _dyn_header(b, True, [8] * 257, [0]))
    _rejected("lit_three_of_1", lit_rule, "oversubscribed literal/length tree", lambda b: _dyn_header(b, True, [1, 1] + [0] * 254 + [1], [0]),
              placements=("first",))
    two = [0] * 257
    two[65] = two[256] = 2
    _rejected("lit_two_of_2", lit_rule, "incomplete literal/length tree", lambda b: _dyn_header(b, True, two, [0]))
    # complete, with 15-bit codes: 1 / 2 + ... + 1 / 2^15 + 1 / 2^15, end-of-block among the longest
    deep = [0] * 257
    for s, l in zip([256] + list(range(65, 80)), [15, 15] + list(range(14, 0, -1))):
        deep[s] = l
    rng = random.Random(204)
    for pl in ("first", "behind_6k"):
        b = _prefix(pl)
        b.dynamic_block([65, 66] + [rng.randrange(65, 80) for _ in range(120)] + [65], True, deep, [0])
        _twin("lit_15_bit_%s" % pl, lit_rule, b, pl)
    b = Builder()  # the single end-of-block code of one bit
    b.dynamic_block([], True, [0] * 256 + [1], [0])
    _twin("lit_one_of_1", lit_rule, b)

    _rejected("dist_three_of_1", dist_rule, "oversubscribed distance tree", lambda b: _dyn_header(b, True, WITH_LEN, [1, 1, 1]))
    _rejected("dist_two_of_2", dist_rule, "incomplete distance tree", lambda b: _dyn_header(b, True, WITH_LEN, [2, 2]))
    _rejected("dist_2_3_3", dist_rule, "incomplete distance tree", lambda b: _dyn_header(b, True, WITH_LEN, [2, 3, 3]), placements=("first",))
    _rejected("dist_none_hlit_258", dist_rule, "empty distance tree with lengths", lambda b: _dyn_header(b, True, WITH_LEN, [0]))
    _rejected("dist_none_hlit_286", dist_rule, "empty distance tree with lengths", lambda b: _dyn_header(b, True, [8] * 226 + [9] * 60, [0, 0]),
              placements=("first",))
    for pl in PLACEMENTS:
        b = _prefix(pl)
        b.dynamic_block([65, (3, 1), 66, (3, 1)], True, WITH_LEN, [1])
        _twin("dist_one_of_1_%s" % pl, dist_rule, b, pl)
    b = Builder()
    b.dynamic_block(b"no distance code, HLIT 257", True, FLAT, [0])
    _twin("dist_none_hlit_257", dist_rule, b)


# ------------------------------------------------------------------ symbols
def _symbol_cases():
    rule = "symbols"

    def fixed(tokens, code):
        def w(b):
            b.put(1, 1), b.put(1, 2)
            assert _emit(b, tokens, db._FIXED_LIT, db._FIXED_DIST)
            b.code(*code)
        return w
    for s in (286, 287):
        _rejected("fixed_lit_%d" % s, rule, "invalid literal/length code", fixed([72, 105], db._FIXED_LIT[s]))
    b = Builder()
    b.fixed_block([72, (258, 1)], True)
    _twin("fixed_lit_285", rule, b)
    for s in (30, 31):
        def w(b, s=s):
            fixed([72, 105], db._FIXED_LIT[257])(b)
            b.code(*db._FIXED_DIST[s])
        _rejected("fixed_dist_%d" % s, rule, "invalid distance code", w)
    b = _prefix("behind_100k")
    b.fixed_block([(3, 24577), (4, 32768)], True)
    _twin("fixed_dist_29", rule, b, "behind_100k")

    def lit_unused(b):
        _dyn_header(b, True, [0] * 256 + [1], [0])
        b.put(0xFFFFF, 20)
    _rejected("dyn_lit_unused_code", rule, "invalid literal/length code", lit_unused)

    def dist_unused(b):
        lit, _ = _dyn_header(b, True, WITH_LEN, [1])
        _emit(b, [65], lit, [])
        _sym(b, lit, 257)
        b.put(0xFFFFF, 20)
    _rejected("dyn_dist_unused_code", rule, "invalid distance code", dist_unused)


def _reach_cases():
    rule = "distance reach"
    rng = random.Random(205)

    def place(name):
        b = Builder()
        if name == "first_token":
            return b, [65]
        b.dynamic_block(rng.randbytes({"at_32768": 32767, "second_block": 2000}[name]), False)
        return b, []
    for name in ("first_token", "at_32768", "second_block"):
        for over in (1, 0):
            b, lead = place(name)
            produced = len(b.plaintext) + len(lead)
            _raw_block(b, lead + [(3, produced + over)] + ([] if over else [66, (258, min(produced + 3, 32768))]), True)
            if over:
                _filler(b)
                _add("reach_%s_plus_1" % name, b.finish(), ZS_DATA_ERROR, "invalid distance code", b.plaintext, rule, "rejected", name)
            else:
                _twin("reach_%s_exact" % name, rule, b, name)
    b = Builder()
    b.dynamic_block(rng.randbytes(32768), False)
    b.dynamic_block([(3, 32768), (258, 32768), 7, (5, 32768)], True)
    _twin("reach_32768_of_32768", rule, b, "at_32768")
    b = _prefix("behind_100k")
    b.dynamic_block([(258, 32768), (3, 32768)], True)
    _twin("reach_32768_behind_100k", rule, b, "behind_100k")


def _trailer_cases():
    rule = "trailer"
    for pl in PLACEMENTS:
        b = _prefix(pl)
        b.fixed_block([84, (4, 1), 85], True)
        z = b.finish()
        _add("trailer_ok_%s" % pl, z, ZS_STREAM_END, None, b.plaintext, rule, "accepted", pl)
        for k in range(4):
            i = len(z) - 4 + k
            _add("trailer_byte_%d_%s" % (k, pl), z[:i] + bytes([z[i] ^ (0x80 >> k)]) + z[i + 1:], ZS_DATA_ERROR, "incorrect data check",
                 b.plaintext, rule, "rejected", pl)
    b = Builder()
    b.fixed_block([], True)
    z = b.finish()
    assert z[-4:] == b"\0\0\0\1"
    _add("trailer_empty_ok", z, ZS_STREAM_END, None, b"", rule, "accepted", "first")
    _add("trailer_empty_flipped", z[:-1] + b"\0", ZS_DATA_ERROR, "incorrect data check", b"", rule, "rejected", "first")


_header_cases()
_block_header_cases()
_bit_length_cases()
_repeat_cases()
_tree_cases()
_symbol_cases()
_reach_cases()
_trailer_cases()
CASES = tuple(_CASES)
NAMES = tuple(c[0] for c in CASES)
_BY_NAME = {c[0]: c for c in CASES}


def case(name):
    return _BY_NAME[name]


def capacity(c):
    return c[4] if c[2] == ZS_STREAM_END else c[4] + SLACK


def messages():
    """Every message the catalogue claims, the truncation sweeps' included."""
    return {c[3] for c in CASES if c[3]} | {"buffer error"}


def paired():
    """The catalogue with every accepted twin next to a rejected case of its rule: rule by rule in the order the rules first
    appear, rejected and accepted cases alternating while both last."""
    out, seen = [], set()
    for c in CASES:
        rule = META[c[0]][0]
        if rule in seen:
            continue
        seen.add(rule)
        rej = [n for n in RULES[rule]["rejected"] if META[n][0] == rule]
        acc = [n for n in RULES[rule]["accepted"] if META[n][0] == rule]
        for k in range(max(len(rej), len(acc))):
            out += [case(n) for n in (rej[k:k + 1] + acc[k:k + 1])]
    assert sorted(c[0] for c in out) == sorted(NAMES)
    return out


# ------------------------------------------------------------------ the sweeps' stream
@functools.lru_cache(maxsize=None)
def sweep():
    """(stream, plaintext, blocks, end of the first dynamic header in bytes): three dynamic blocks, a stored block, a fixed
    block with a 258-long overlapping match, a final dynamic block, the trailer."""
    rng = random.Random(206)
    b = Builder()
    for k in range(3):
        b.dynamic_block(list(rng.randbytes(500)) + [(258, 1 + 150 * k), 7, (31, 499)] + list(rng.randbytes(40)), False)
    b.stored_block(rng.randbytes(300), False)
    b.fixed_block([88, (258, 1), 89, (10, 200), 90], False)
    b.dynamic_block(list(rng.randbytes(400)) + [(258, 700), (40, 3), (258, 258)] + list(rng.randbytes(30)), True)
    z = b.finish()
    # the first block's header ends where its first symbol begins: the same code lengths give the same header
    _, lit_lengths, dist_lengths, _ = b.lengths[0]
    e = Builder()
    bits = e.dynamic_block([], False, lit_lengths, dist_lengths)
    header_bits = bits - lit_lengths[256]
    assert 2400 <= len(z) <= 3100 and 3500 <= len(b.plaintext) <= 4600, (len(z), len(b.plaintext))
    return z, bytes(b.plaintext), tuple(b.blocks), (16 + header_bits + 7) // 8


def sweep_single_cuts():
    """Cuts to run alone, for the message: every byte of the first dynamic header (and the two header bytes), one byte
    inside each block's symbols or data, inside the stored block's LEN / NLEN, and inside the trailer."""
    z, _, blocks, header_end = sweep()
    cuts = set(range(header_end + 1))
    for kind, start, bits in blocks:
        cuts.add((start + bits // 2) // 8)
        if kind == "stored":
            cuts.add((start + 3 + 7) // 8 + 2)
    cuts |= {len(z) - 5, len(z) - 4, len(z) - 2, len(z) - 1}
    return sorted(cuts)
