"""The filter rules of include/zsgpu.h (zs_chunk_filters) as a numpy model on top of tests/chunk_cases.py, and the cases the filter
tests share: delta over a padded chunk, big-endian elements, the whole encode / decode chain of a chunk, HDF5's Fletcher-32 as the
literal loop of H5_checksum_fletcher32 (the yardstick) beside the closed form the kernel uses, and the catalogue of grids, filter
combinations and failing chunks.  Written from the header's text, not from the library."""
import itertools
import struct

import numpy as np

import chunk_cases as cc
from chunk_cases import STORED, UNSHUFFLED, ZS_DATA_ERROR

UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


# ------------------------------------------------------------------ Fletcher-32
def fletcher32_loop(d):
    """H5_checksum_fletcher32, literally: the yardstick"""
    d = bytes(d)
    M = 0xFFFFFFFF
    s1 = s2 = 0
    words = len(d) // 2
    p = 0
    while words:
        t = min(words, 360)
        words -= t
        for _ in range(t):
            s1 = (s1 + ((d[p] << 8) | d[p + 1])) & M
            p += 2
            s2 = (s2 + s1) & M
        s1 = (s1 & 0xFFFF) + (s1 >> 16)
        s2 = (s2 & 0xFFFF) + (s2 >> 16)
    if len(d) % 2:
        s1 = (s1 + (d[p] << 8)) & M
        s2 = (s2 + s1) & M
        s1 = (s1 & 0xFFFF) + (s1 >> 16)
        s2 = (s2 & 0xFFFF) + (s2 >> 16)
    s1 = (s1 & 0xFFFF) + (s1 >> 16)
    s2 = (s2 & 0xFFFF) + (s2 >> 16)
    return ((s2 << 16) | s1) & M


def fletcher32_sums(d):
    """the closed form's triple of a run of bytes: (sum of the words, sum of (n - i) * word i, any word non-zero), the sums
    modulo 65535; an odd last byte is a word with a zero low byte"""
    d = bytes(d)
    if len(d) % 2:
        d += b"\0"
    w = np.frombuffer(d, ">u2").astype(object)
    n = len(w)
    a1 = int(sum(w)) % 65535
    a2 = int(sum((n - i) * int(x) for i, x in enumerate(w))) % 65535
    return a1, a2, int(any(w))


def fletcher32_combine(a, b, m_words):
    """a tile's triple followed by a tile of m_words words with triple b"""
    return (a[0] + b[0]) % 65535, (a[1] + m_words * a[0] + b[1]) % 65535, a[2] | b[2]


def fletcher32_finish(t):
    s1, s2 = (v if v else (0xFFFF if t[2] else 0) for v in t[:2])
    return (s2 << 16) | s1


def fletcher32_closed(d):
    return fletcher32_finish(fletcher32_sums(d))


def fletcher32_fast(d):
    """the closed form with numpy sums, for long inputs (tests/test_chunk_filter_host.py holds it against the loop)"""
    d = bytes(d)
    if len(d) % 2:
        d += b"\0"
    w = np.frombuffer(d, ">u2").astype(np.uint64)
    n = len(w)
    a1 = a2 = 0
    for at in range(0, n, 1 << 16):  # (65536 words of 16 bits times a weight below 2^31: inside uint64)
        part = w[at:at + (1 << 16)]
        a1 += int(part.sum())
        a2 += int((part * (np.uint64(n - at) - np.arange(len(part), dtype=np.uint64))).sum())
    return fletcher32_finish((a1 % 65535, a2 % 65535, int(w.any())))


def with_checksum(blob):
    return bytes(blob) + struct.pack("<I", fletcher32_loop(blob))


# ------------------------------------------------------------------ delta and the byte order
def delta_encode(data, es):
    """enc[0] = x[0], enc[k] = x[k] - x[k-1], wrapping, over len // es little-endian elements; the leftover bytes unchanged"""
    data = bytes(data)
    count = len(data) // es
    x = np.frombuffer(data[:count * es], "<u%d" % es)
    enc = x.copy()
    enc[1:] = x[1:] - x[:-1]
    return enc.astype("<u%d" % es).tobytes() + data[count * es:]


def delta_decode(data, es):
    data = bytes(data)
    count = len(data) // es
    x = np.frombuffer(data[:count * es], "<u%d" % es)
    return np.cumsum(x, dtype=UINT[es]).astype("<u%d" % es).tobytes() + data[count * es:]


def byteswap(data, es):
    """every element's bytes reversed"""
    return np.frombuffer(bytes(data), np.uint8).reshape(-1, es)[:, ::-1].tobytes()


NONE = {"delta": 0, "byte_order": 0, "fletcher32": 0}


def filters(delta=0, byte_order=0, fletcher32=0):
    return {"delta": int(delta), "byte_order": int(byte_order), "fletcher32": int(fletcher32)}


def all_filters():
    return [filters(d, b, f) for d, b, f in itertools.product((0, 1), repeat=3)]


def filtered_chunk(data, g, f, c, shuffled=None, pad=None):
    """chunk c of the array as it is handed to deflate: padded with fill, delta, byte order, shuffle"""
    es = g["elem_size"]
    raw = cc.chunk_of(data, g, c, shuffled=False, pad=pad)
    if f["delta"]:
        raw = delta_encode(raw, es)
    if f["byte_order"] and es > 1:
        raw = byteswap(raw, es)
    return cc.shuffle(raw, es) if (g["shuffle"] if shuffled is None else shuffled) else raw


def unfiltered_chunk(blob, g, f, shuffled=None):
    """the inverse: the bytes behind inflate to the chunk's plain little-endian elements"""
    es = g["elem_size"]
    raw = cc.unshuffle(blob, es) if (g["shuffle"] if shuffled is None else shuffled) else bytes(blob)
    if f["byte_order"] and es > 1:
        raw = byteswap(raw, es)
    return delta_decode(raw, es) if f["delta"] else raw


def stored_bytes(blob, f):
    """what is stored for a chunk whose last bytes in front of the checksum are `blob`"""
    return with_checksum(blob) if f["fletcher32"] else bytes(blob)


def encoded_chunks(data, g, f, level=6, pad=None):
    """every chunk of the array as its writer would store it"""
    return [stored_bytes(cc.compress(filtered_chunk(data, g, f, c, pad=pad), g["wrap"], level), f) for c in range(cc.n_chunks(g))]


def decoded_chunk(stored, g, f, flags=0):
    """a stored chunk back to its plain elements, the checksum checked"""
    if f["fletcher32"]:
        assert len(stored) >= 4 and struct.unpack("<I", stored[-4:])[0] == fletcher32_loop(stored[:-4])
        stored = stored[:-4]
    blob = stored if flags & STORED else cc.decompress(stored, g["wrap"])[0]
    return unfiltered_chunk(blob, g, f, shuffled=False if flags & UNSHUFFLED else None)


# ---- the failing variants that Fletcher-32 adds, for a chunk whose filtered bytes are `blob`: (name, bytes, flags, code, message)
def failing_checksum_chunks(blob, g):
    good = with_checksum(cc.compress(blob, g["wrap"]))
    out = []
    bad = bytearray(good)
    bad[len(good) // 2 - 2] ^= 0x10
    out.append(("a flipped bit in the stream", bytes(bad), 0, ZS_DATA_ERROR, "incorrect chunk checksum"))
    bad = bytearray(good)
    bad[-2] ^= 0x01
    out.append(("a flipped bit in the checksum", bytes(bad), 0, ZS_DATA_ERROR, "incorrect chunk checksum"))
    bad = bytearray(with_checksum(blob))
    bad[3] ^= 0x80
    out.append(("a flipped bit in a STORED chunk", bytes(bad), STORED, ZS_DATA_ERROR, "incorrect chunk checksum"))
    for n in range(4):
        out.append(("len %d" % n, good[:n], 0, ZS_DATA_ERROR, "incorrect chunk length"))
    out.append(("a right but short stream, its checksum right", with_checksum(cc.compress(blob[:-g["elem_size"]], g["wrap"])), 0, ZS_DATA_ERROR, "incorrect chunk length"))
    out.append(("a STORED chunk without its checksum", blob, STORED, ZS_DATA_ERROR, "incorrect chunk length"))
    return out


def ramp_array(g, seed):
    """integers that rise slowly (what delta is for) with steps that wrap: elements of elem_size bytes, little-endian"""
    es = g["elem_size"]
    n = cc.array_bytes(g) // es
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.integers(0, 5, n, dtype=np.uint64), dtype=np.uint64) + np.uint64((1 << (8 * es)) - 20 if es < 8 else (1 << 64) - 20)
    return x.astype(UINT[es]).astype("<u%d" % es).tobytes()
