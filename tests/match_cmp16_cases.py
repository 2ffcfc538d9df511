"""Inputs for the match kernel's 16-byte first compare (zlibstream_amd/csrc/zs_kernels.hip, match_walk, ZS_CMP16): streams whose
deciding candidate has exactly 7 .. 258 equal bytes.  Every input is filler in which no three bytes repeat (64 letters: no
chance matches, and Huffman codes keep the blocks from being stored) around copies of one 300-byte string S, of bytes the
filler does not use, cut to the wanted length and followed by a differing byte; all copies of at least 6 bytes share S's bucket
(bytes 2 .. 5), so the probe -- S in full -- meets them on one chain, nearest first.

CASES[name] = (data, claim): claim(tokens, level) says what the reference's stream must hold for the case to be the edge it is
meant to be (tokens: {position: (length, distance)}, tests/match_cases.py); tests/test_match_cmp16_cases.py holds the claims
against the oracle on the CPU, tests/test_gpu_match_cmp16.py compares the device's bytes with the oracle's."""
import random

LEVELS = (4, 6, 9)
LENGTHS = (7, 8, 9, 15, 16, 17, 23, 24, 25, 257, 258)
NICE = {4: 16, 6: 128, 9: 258}
CHAIN = {4: 16, 6: 128, 9: 4096}
GOOD = {4: 4, 6: 8, 9: 32}

_R = random.Random(20240616)
S = bytes(_R.randrange(128, 256) for _ in range(300))
_SEEN = set()  # the filler's byte triples in the case being built
_LAST = bytearray(b"  ")  # the filler's last two bytes


def fill(n):
    out = bytearray(_LAST)
    tries = 0
    while len(out) < n + 2:
        b = _R.randrange(0x20, 0x60)
        tries += 1
        assert tries < 100 * (n + 2), "the filler has run out of fresh triples"
        if (out[-2], out[-1], b) not in _SEEN:
            _SEEN.add((out[-2], out[-1], b))
            out.append(b)
    _LAST[:] = out[-2:]
    return bytes(out[2:])


def _copy(length):
    """S's first `length` bytes and a byte that differs from the next one of S"""
    return S[:length] + bytes([S[length] ^ 0x15])


def _chain(*lengths, lead=700):
    """copies of the given lengths, farthest first, then the probe; returns data, the probe's position, the copies' distances"""
    data, at = fill(lead), []
    for n in lengths:
        at.append(len(data))
        data += _copy(n) + fill(200)
    data += fill(100)
    probe = len(data)
    return data + S + fill(600), probe, [probe - a for a in at]


def _first(n):
    data, p, (d,) = _chain(n)
    return data, lambda t, level: t.get(p) == (n, d)


def _later_beats_shorter(n):
    short = max(6, n - 3)  # (at 254 and 255 bytes it is nice enough for levels 4 and 6, which stop there)
    data, p, (far, near) = _chain(n, short)
    return data, lambda t, level: t.get(p) == ((short, near) if short >= NICE[level] else (n, far))


def _tie_keeps_the_nearer(n):
    data, p, (_, near) = _chain(n, n)
    return data, lambda t, level: t.get(p) == (n, near)


def _nice_then_longer(n):
    """a nearer copy of n bytes in front of a longer one: at level 4 (nice 16) 16 and 17 bytes end the walk, 9 .. 15 do not"""
    data, p, (far, near) = _chain(n + 20, n)
    return data, lambda t, level: t.get(p) == ((n, near) if n >= NICE[level] else (n + 20, far))


def _zeros_at_the_end(before_end, n):
    """zero bytes up to the end of the input: the position `before_end` bytes in front of the end has n zeros behind it in the run
    and staged zeros behind the end; the stream's last match must end with the input"""
    data = fill(900) + bytes(n + before_end)
    return data, lambda t, level: max(p + l for p, (l, _) in t.items()) == len(data)


def _across_the_tile(n, at):
    """the probe `at` bytes in front of position 16384, its candidate in the tile before"""
    head = fill(9000)
    c = len(head)
    head += _copy(n)
    data = head + fill(16384 - at - len(head))
    p = len(data)
    assert p == 16384 - at
    return data + S + fill(2500), lambda t, level: t.get(p) == (n, p - c)


def _frozen_quarter(n):
    """Level 6: chain >> 2 = 32 copies of 6 bytes and two more in front of a copy of n bytes (9 .. 15): the improvement comes
    behind the quarter budget and freezes that record at 6 bytes.  A match of good_length = 8 bytes at the position before the
    probe makes the parse ask for the quarter budget there, and since n > 8 > 6 that earlier match is kept only if the quarter
    record is the frozen one.  (The parse shows the quarter record at level 6 only: level 4 never searches behind a match of
    good_length, max_lazy being 4 too, and at level 9 good_length is 32, above every length in bytes 8 .. 15.  The records of
    all three levels are held against the plain walk on the host, tests/cpp/test_match_sched.cpp.)"""
    z = bytes([S[0] ^ 0x33])
    data = fill(500)
    zc = len(data)
    data += z + S[:GOOD[6] - 1] + bytes([S[GOOD[6] - 1] ^ 0x15]) + fill(40) + _copy(n) + fill(30)
    for _ in range((CHAIN[6] >> 2) + 2):
        data += _copy(6) + fill(3)
    data += fill(100)
    pz = len(data)
    return data + z + S + fill(600), lambda t, level: level != 6 or t.get(pz) == (GOOD[6], pz - zc)


class _Cases(dict):
    def __setitem__(self, name, case):
        _SEEN.clear()  # (the builder has run: the next case starts afresh)
        dict.__setitem__(self, name, case)


def _cases():
    out = _Cases()
    for n in LENGTHS:
        out["first_%d" % n] = _first(n)
        out["later_%d" % n] = _later_beats_shorter(n)
        out["tie_%d" % n] = _tie_keeps_the_nearer(n)
    for n in (9, 12, 15, 16, 17):
        out["nice_%d" % n] = _nice_then_longer(n)
    for before_end in range(9, 18):
        for n in LENGTHS:
            out["end_%d_%d" % (before_end, n)] = _zeros_at_the_end(before_end, n)
    for n in (9, 16, 24, 258):
        for at in (3, 12, 20):
            out["tile_%d_%d" % (n, at)] = _across_the_tile(n, at)
    for n in (9, 12, 15):
        out["frozen_L6_%d" % n] = _frozen_quarter(n)
    return out


CASES = _cases()
PERIODIC = (b"QRSTUVW" * 12000)[:80000] + _first(16)[0]
_REF = {}


def ref(oracle, name, level):
    if (name, level) not in _REF:
        _REF[(name, level)] = oracle.compress(CASES[name][0], level, 0)
    return _REF[(name, level)]
