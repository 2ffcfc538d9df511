"""Inputs for the encoder's back end -- the tree kernel (K7, zs_trees_kernel / build_tree_wave), block placement (K8,
zs_offsets_kernel) and bit packing (K9, zs_emit_bits_kernel) -- at the edges that the corpus and the fuzzers do not reach.

A case is (name, data, level, strategy, claim).  The claim is a predicate over tests/deflate_reader.py's view of the ORACLE's
stream of that input: it says why the case is here (the 15-bit repair ran; the stored block starts at bit phase 5; ...).
tests/test_emit_cases.py holds every claim against the oracle on the CPU; tests/test_gpu_emit_cases.py then asks the device
for the oracle's bytes.  A claim is never evaluated on the device's stream.  Seeds and sizes were tuned on the CPU until the
claims held, and are frozen.

Under HuffmanOnly (HO) nothing is matched: a block is the next 16383 bytes (kBlockSyms) and its literal histogram is their byte
histogram, which an input can therefore set exactly.  HLIT and HDIST are counts here (the header fields are HLIT - 257 and
HDIST - 1); Build_tree forces two codes, so the encoder's smallest HDIST is 2, a field value of 1."""
import functools
import random

import deflate_reader as dr
from deflate_builder import DIST_BASE, LEN_BASE

DEFAULT, FILTERED, HO, RLE, FIXED = 0, 1, 2, 3, 4
BLOCK = 16383  # kBlockSyms


def _fib(n, a=1, b=2):
    out = []
    while len(out) < n:
        out.append(a)
        a, b = b, a + b
    return out


def _from_counts(counts, seed, values=None):
    """Bytes with exactly these counts, shuffled: counts[i] of values[i] (of byte i without values)."""
    rng = random.Random(seed)
    values = list(values) if values is not None else list(range(len(counts)))
    d = [v for v, c in zip(values, counts) for _ in range(c)]
    rng.shuffle(d)
    return bytes(d)


def _skewed(seed, n, k=48):
    """n bytes of k letters, the i-th with weight 1 / (i + 1): compressible whatever the strategy, no byte pattern."""
    rng = random.Random(seed)
    return bytes(rng.choices(range(97 - 32, 97 - 32 + k), [1.0 / (i + 1) for i in range(k)], k=n))


def _lit_repair(b):
    return dr.repair_ran(b.lit_hist, b.lit_lengths, 15)


def _dist_repair(b):
    return dr.repair_ran(b.dist_hist, b.dist_lengths, 15)


def _bl_repair(b):
    return dr.repair_ran(dr.bl_hist(b), b.bl_lengths, 7)


def _one_dynamic(blocks, pred):
    return len(blocks) == 1 and blocks[0].kind == "dynamic" and pred(blocks[0])


def _used(hist):
    return [i for i, f in enumerate(hist) if f]


# ------------------------------------------------------------------ the trees: overflow, ties, forced codes
def _tree_cases():
    out = []
    # 18 byte values + END_BLOCK's 1 in front: 1, 1, 2, 3, 5, ... has ties at the bottom and still a depth of 18; the repair
    # leaves six 15-bit codes.  (Exact Fibonacci counts 1, 1, 2, ... *plus* END_BLOCK tie into a shallow tree.)
    out.append(("lit_overflow", _from_counts(_fib(18), 201), 6, HO, lambda bl: _one_dynamic(bl, lambda b: _lit_repair(b) and b.lit_lengths.count(15) == 6)))
    out.append(("lit_overflow_by_one", _from_counts(_fib(16), 202), 6, HO, lambda bl: _one_dynamic(bl, _lit_repair)))
    out.append(("lit_natural_15", _from_counts(_fib(15), 203), 6, HO,
                lambda bl: _one_dynamic(bl, lambda b: max(b.lit_lengths) == 15 and dr.code_cost(b.lit_hist, b.lit_lengths) == dr.optimal_cost(b.lit_hist))))
    out.append(("bl_overflow", _bl_overflow_input(), 6, HO, lambda bl: _one_dynamic(bl, _bl_repair)))
    # Build_tree's "force at least two codes": the distance tree with no, one low and one high code in use
    out.append(("dist_none", _skewed(204, 3000), 6, HO, lambda bl: _one_dynamic(bl, lambda b: not any(b.dist_hist) and b.dist_lengths == [1, 1] and b.hlit == 257)))
    rng = random.Random(205)
    runs = b"".join(bytes([rng.randrange(256)]) * rng.randrange(4, 300) for _ in range(200))
    out.append(("dist_code0_rle", runs, 6, RLE, lambda bl: _one_dynamic(bl, lambda b: _used(b.dist_hist) == [0] and b.dist_lengths == [1, 1])))
    out.append(("dist_code0_run", b"q" * 5000, 6, DEFAULT, lambda bl: len(bl) == 1 and _used(bl[0].dist_hist) == [0]))
    out.append(("dist_code1", b"xy" * 2500, 6, DEFAULT, lambda bl: len(bl) == 1 and _used(bl[0].dist_hist) == [1]))
    out.append(("dist_code9", (rng.randbytes(29) * 400)[:9000], 6, DEFAULT,
                lambda bl: _one_dynamic(bl, lambda b: _used(b.dist_hist) == [9] and b.dist_lengths == [1] + [0] * 8 + [1])))
    out.append(("empty_input", b"", 6, DEFAULT, lambda bl: len(bl) == 1 and bl[0].kind == "fixed" and bl[0].symbols == []))
    out.append(("one_byte", b"Z", 6, DEFAULT, lambda bl: len(bl) == 1 and bl[0].kind == "fixed" and bl[0].symbols == [90]))
    out.append(("one_byte_ho", b"Z", 6, HO, lambda bl: len(bl) == 1 and bl[0].symbols == [90]))
    # a symbol count that is a multiple of kBlockSyms.  Levels 1-3 close a full block at once and end the stream with a block of
    # no symbol but END_BLOCK; levels 4-9 close it when the next symbol arrives, so there the last block is the full one.  (The
    # other blocks of 0 symbols are empty_input's and the flush markers'.)
    for k in (1, 2):
        out.append(("empty_last_block_%d" % (k * BLOCK), _skewed(206 + k, k * BLOCK), 1, HO,
                    lambda bl, k=k: len(bl) == k + 1 and all(len(b.symbols) == BLOCK for b in bl[:-1]) and bl[-1].symbols == [] and bl[-1].kind == "fixed"))
        out.append(("full_last_block_%d" % (k * BLOCK), _skewed(206 + k, k * BLOCK), 6, HO,
                    lambda bl, k=k: len(bl) == k and all(len(b.symbols) == BLOCK and b.kind == "dynamic" for b in bl)))
    return out


def _bl_overflow_input():
    """Found by a seeded search over skewed histograms (tests/test_emit_cases.py holds the claim): literal code lengths whose
    counts are so uneven that the bit-length tree's natural depth passes 7."""
    return _bl_candidate(_BL_SEED)


_BL_SEED = 36  # cost 634 against an optimal 627


def _bl_candidate(seed):
    rng = random.Random(9000 + seed)
    k = rng.randrange(20, 200)
    vals = rng.sample(range(256), k)
    counts = [max(1, int(rng.paretovariate(0.6))) for _ in range(k)]
    scale = max(1.0, sum(counts) / 16000.0)
    return _from_counts([max(1, int(c / scale)) for c in counts], seed, vals)[:BLOCK - 1]


# ------------------------------------------------------------------ alphabet extent
def _match(out, length, dist, rng):
    """Append a guard byte, `length` bytes that repeat what lies `dist` back, and a byte that ends the repeat: the lazy parse
    sees one match (length, dist) between two literals."""
    out.append(rng.choice([v for v in range(256) if v != out[len(out) - dist]]))
    for _ in range(length):
        out.append(out[len(out) - dist])
    out.append(rng.choice([v for v in range(256) if v != out[len(out) - dist]]))


def _all_codes_input():
    """The reference hashes the four bytes at str + 2 .. str + 5, so what it finds by content is six bytes long or longer.
    Lengths 3 and 4 are matches between strings whose hashed bytes differ and share a bucket (CRC-32C, 15 bits: 63 31 32 33,
    63 ee ed dd and 63 31 7f a3 do); length 5 is the stream's last match, cut by the end of the input, whose hash reads the
    zero behind it."""
    rng = random.Random(210)
    out = bytearray(rng.randbytes(40000))  # two blocks of literals and the start of the third: every byte value, sources for far matches
    for dc in range(30):
        _match(out, LEN_BASE[dc if 3 <= dc <= 28 else 10 + dc % 3], DIST_BASE[dc] + (dc > 3), rng)
    a, b = 0x61, 0x62
    for other in (b"\xee\xed\xdd", b"\x31\x7f\xa3"):
        out += bytes([a, b]) + b"\x63\x31\x32\x33" + rng.randbytes(5) + bytes([a, b, 0x63]) + other + rng.randbytes(5)
        a, b = a + 2, b + 2
    out += b"vwxyz\0" + rng.randbytes(5) + b"vwxyz"
    return bytes(out)


_FLAT_SEED = 211


def _extent_cases():
    out = []
    out.append(("all_codes", _all_codes_input(), 6, DEFAULT,
                lambda bl: any(b.kind == "dynamic" and b.hlit == 286 and b.hdist == 30 and all(b.lit_hist) and all(b.dist_hist) for b in bl)))
    # a run of all 286 literal/length codes with the only distance code Rle knows
    rng = random.Random(213)
    runs = bytearray(range(256))
    for lc in range(29):
        runs += bytes([rng.randrange(256)]) * (LEN_BASE[lc] + 1) + bytes([255 - runs[-1]])
    out.append(("all_lengths_rle", bytes(runs) + _skewed(214, 4000), 6, RLE, lambda bl: _one_dynamic(bl, lambda b: all(b.lit_hist) and _used(b.dist_hist) == [0])))
    # 256 literals of equal count: every comparison of the heap is a tie.  Alone they would be stored, so a run behind them
    # pays for the block: a stored block's bytes do not show its trees
    flat = bytearray(_from_counts([8] * 256, _FLAT_SEED))
    flat.remove(0)
    out.append(("flat_256", bytes(flat) + bytes(258 * 40 + 1), 6, DEFAULT,
                lambda bl: _one_dynamic(bl, lambda b: b.lit_hist[:256] == [8] * 256 and _used(b.dist_hist) == [0])))
    pw = [c for k in range(2, 12) for c in (2 ** k - 1, 2 ** k, 2 ** k + 1)]
    out.append(("pow2_counts", _from_counts(pw, 212, range(40, 70)), 6, HO,
                lambda bl: _one_dynamic(bl, lambda b: [f for f in b.lit_hist[:256] if f] == pw)))
    return out


# ------------------------------------------------------------------ scan_tree / send_tree
def _layout_input(plan, seed):
    """plan: ("gap", n) leaves n byte values unused; ("run", n, f) uses the next n byte values f times each."""
    counts, v = [0] * 256, 0
    for p in plan:
        if p[0] == "run":
            for _ in range(p[1]):
                counts[v] = p[2]
                v += 1
        else:
            v += p[1]
    assert v <= 256
    return _from_counts(counts, seed)


def _sent(b):
    return set(b.sent)


def _follows(b, first, second):
    """`second` is sent directly behind `first` (predicates over (symbol, repeat))."""
    return any(first(x) and second(y) for x, y in zip(b.sent, b.sent[1:]))


def _gaps(b):
    """Runs of unused symbols between used ones in the literal/length lengths, and runs of equal non-zero lengths."""
    zero, same, i, L = set(), set(), 0, b.lit_lengths + b.dist_lengths
    while i < len(L):
        j = i
        while j < len(L) and L[j] == L[i]:
            j += 1
        (zero if L[i] == 0 else same).add(j - i)
        i = j
    return zero, same


def _scan_cases():
    out = []
    # runs of 3, 4, 6, 7, 8 and 13 equal lengths (the counts alternate so that neighbours differ), gaps of 2, 3, 10, 11 and 138
    # (counts that are exact powers of two leave the code no choice: count 4 is 5 bits, count 1 -- END_BLOCK's too -- 7, count 32 is 2;
    # the three symbols in front of END_BLOCK make 128 of it)
    plan_a = [("run", 3, 4), ("gap", 2), ("run", 4, 1), ("gap", 3), ("run", 6, 4), ("gap", 10), ("run", 7, 1), ("gap", 11), ("run", 8, 4),
              ("gap", 138), ("run", 13, 1), ("gap", 5), ("run", 1, 32), ("gap", 42), ("run", 3, 1)]
    out.append(("scan_runs_gap138", _layout_input(plan_a, 220), 6, HO, lambda bl: _one_dynamic(bl, lambda b: (
        _gaps(b)[0] >= {2, 3, 10, 11, 138} and _gaps(b)[1] >= {3, 4, 6, 7, 8, 13} and
        _sent(b) >= {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)} and
        _follows(b, lambda x: 1 <= x[0] <= 15, lambda y: y[0] == 16) and _follows(b, lambda x: x[0] == 16, lambda y: y[0] == 16)))))
    for gap in (139, 140):  # 138 and then one or two explicit zeros: the repeat code's largest count, exceeded
        plan = [("run", 5, 40), ("gap", gap), ("run", 9, 20)]
        out.append(("scan_gap%d" % gap, _layout_input(plan, 220 + gap), 6, HO, lambda bl, gap=gap: _one_dynamic(bl, lambda b: (
            gap in _gaps(b)[0] and _follows(b, lambda x: x == (18, 138), lambda y: y == (0, 1))))))
    return out


# ------------------------------------------------------------------ K8: stored blocks at every bit phase
STORED_PHASE_VARIANTS = 12


def _stored_phase_input(v):
    text, rnd = _skewed(230, BLOCK), random.Random(231).randbytes(BLOCK)
    first = bytearray(text)
    rng = random.Random(232 + v)
    for _ in range(v):  # a few bytes of the first block changed: its length in bits moves, and the stored header with it
        first[rng.randrange(BLOCK)] = 97 - 32 + rng.randrange(48)
    return bytes(first) + rnd + text


def _stored_phase_cases():
    return [("stored_phase_%02d" % v, _stored_phase_input(v), 6, HO,
             lambda bl: [b.kind for b in bl] == ["dynamic", "stored", "dynamic"] and bl[1].len == BLOCK) for v in range(STORED_PHASE_VARIANTS)]


# ------------------------------------------------------------------ K9: tiles of 2048 symbols
TILE_SIZES = (2046, 2047, 2048, 2049, 4095, 4096, 4097, 16382, 16383, 16384)


def _tile_cases():
    # a block has n + 1 symbols with END_BLOCK: 2048 bytes leave END_BLOCK alone in the last tile
    return [("tile_%d" % n, _skewed(240, n), 6, HO,
             lambda bl, n=n: bl[0].kind == "dynamic" and len(bl[0].symbols) == min(n, BLOCK) and len(bl) == 1 + (n > BLOCK)) for n in TILE_SIZES]


# ------------------------------------------------------------------ the distance tree's repair; the longest symbols
def _periodic_segments(rng, plan, out):
    """plan: [(distance, k)] -- `distance` fresh random bytes, repeated to a length of distance + 258 * k: k matches (258, distance)."""
    for d, k in plan:
        seg = rng.randbytes(d)
        out += (seg * ((d + 258 * k) // d + 1))[:d + 258 * k]


def _dist_overflow_input():
    rng = random.Random(250)
    out = bytearray()
    _periodic_segments(rng, list(zip([DIST_BASE[c] for c in range(16, -1, -1)], _fib(17, 1, 1))), out)
    assert len(out) == 1079349
    return bytes(out)


def _long_symbols_input():
    """Far matches with rare length codes (131..257: 5 extra bits) and distance codes 26..29 (12 and 13 extra bits) in front
    of a block built like dist_overflow, which makes their distance codes the rarest: the longest symbols the format has, behind
    literals of 8 and 9 bits at every position modulo 8."""
    rng = random.Random(_LONG_SEED)
    out = bytearray(rng.randbytes(40000))
    far = [(29, 257), (28, 227), (27, 195), (27, 163), (26, 131), (26, 200), (26, 250)]
    for i, (dc, length) in enumerate(far):
        out += rng.randbytes(i + 1)
        _match(out, length, DIST_BASE[dc] + 5 + i, rng)
    _periodic_segments(rng, list(zip([DIST_BASE[c] for c in range(11, -1, -1)], _fib(12, 5, 8))), out)
    return bytes(out)


_LONG_SEED = 260


def _deep_cases():
    out = []
    out.append(("dist_overflow", _dist_overflow_input(), 6, DEFAULT,
                lambda bl: _one_dynamic(bl, lambda b: _dist_repair(b) and b.dist_hist[:17] == _fib(17, 1, 1)[::-1] and b.dist_lengths.count(15) == 4)))
    out.append(("long_symbols", _long_symbols_input(), 6, DEFAULT, lambda bl: max(dr.k9_max_pending(b) for b in bl if b.kind != "stored") >= 57))
    return out


# levels and strategies at which dist_overflow's claim was probed as well; at levels 1-3 the parse differs and nothing overflows:
# there the case runs for its bytes alone
DIST_OVERFLOW_ALSO = ((4, DEFAULT), (9, DEFAULT), (6, FILTERED))
DIST_OVERFLOW_BYTES_ONLY = ((1, DEFAULT), (3, DEFAULT))


# ------------------------------------------------------------------ flushes: one block of each kind in front of the marker
def flush_cases():
    """(name, data, level, strategy, kind of the block a Write of `data` ends in) for the flush tests: lit_overflow's END_BLOCK
    code is 15 bits long (last_eob_len of the flush accounting), a Fixed block's 7, a stored block's 8."""
    return [("lit_overflow", case("lit_overflow")[1], 6, HO, "dynamic"), ("fixed", _skewed(270, 3000), 6, FIXED, "fixed"),
            ("stored", random.Random(271).randbytes(3000), 6, DEFAULT, "stored")]


# ------------------------------------------------------------------ block-type sweeps
SWEEP_MAX = 512
SWEEP_SETTINGS = ((1, DEFAULT), (6, DEFAULT), (6, HO), (6, FIXED))


@functools.lru_cache(maxsize=None)
def sweep_inputs():
    """{generator: [its first n bytes for n = 0..512]}: random bytes, four symbols, one repeated byte."""
    rnd = random.Random(280).randbytes(SWEEP_MAX)
    low = bytes(random.Random(281).choices(b"acgt", [8, 4, 2, 1], k=SWEEP_MAX))
    one = b"\x55" * SWEEP_MAX
    return {g: [d[:n] for n in range(SWEEP_MAX + 1)] for g, d in (("random", rnd), ("four_symbols", low), ("one_byte", one))}


def sweep_claim(kinds, strategy):
    """kinds: {generator: [kind of the only block at n = 0..512]} of one (level, strategy)."""
    seen = {k for ks in kinds.values() for k in ks}
    pairs = {frozenset((a, b)) for ks in kinds.values() for a, b in zip(ks, ks[1:]) if a != b}
    if strategy == FIXED:
        return "dynamic" not in seen and frozenset(("fixed", "stored")) in pairs
    return seen == {"stored", "fixed", "dynamic"} and pairs >= {frozenset(("fixed", "stored")), frozenset(("fixed", "dynamic"))}


# ------------------------------------------------------------------ the catalogue
@functools.lru_cache(maxsize=None)
def catalogue():
    cases = _tree_cases() + _extent_cases() + _scan_cases() + _stored_phase_cases() + _tile_cases() + _deep_cases()
    assert [c[0] for c in cases] == case_names()
    return tuple(cases)


def case_names():
    """The catalogue's names without building it (for parametrised tests)."""
    return (["lit_overflow", "lit_overflow_by_one", "lit_natural_15", "bl_overflow", "dist_none", "dist_code0_rle", "dist_code0_run", "dist_code1",
             "dist_code9", "empty_input", "one_byte", "one_byte_ho", "empty_last_block_16383", "full_last_block_16383", "empty_last_block_32766", "full_last_block_32766", "all_codes", "all_lengths_rle", "flat_256",
             "pow2_counts", "scan_runs_gap138", "scan_gap139", "scan_gap140"] + ["stored_phase_%02d" % v for v in range(STORED_PHASE_VARIANTS)] +
            ["tile_%d" % n for n in TILE_SIZES] + ["dist_overflow", "long_symbols"])


def case(name):
    return next(c for c in catalogue() if c[0] == name)
