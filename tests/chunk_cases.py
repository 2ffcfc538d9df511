"""The chunked-array rules of include/zsgpu.h as a numpy model, and the cases the chunk tests share: the shuffle filter of HDF5
and numcodecs, a grid's chunks cut out of an array with padding, chunks placed into an array, chunk builders for the three
containers through Python's zlib and gzip, and the failing variants.  Written from the header's text, not from the library."""
import gzip
import itertools
import struct
import zlib

import numpy as np

WRAP_ZLIB, WRAP_RAW, WRAP_GZIP = 0, 1, 2
STORED, UNSHUFFLED, SKIP, ABSENT = 1, 2, 4, 8
ZS_OK, ZS_STREAM_END, ZS_NEED_DICT, ZS_STREAM_ERROR, ZS_DATA_ERROR, ZS_MEM_ERROR, ZS_BUF_ERROR = 0, 1, 2, -2, -3, -4, -5


def grid(shape, chunks, elem_size, shuffle=True, wrap=WRAP_ZLIB, fill=None):
    fill = bytes(elem_size) if fill is None else bytes(fill)
    assert len(fill) == elem_size
    return {"shape": tuple(shape), "chunks": tuple(chunks), "elem_size": elem_size, "shuffle": shuffle, "wrap": wrap, "fill": fill}


def cells(g):
    return tuple(-(-s // c) for s, c in zip(g["shape"], g["chunks"]))


def n_chunks(g):
    return int(np.prod(cells(g), dtype=object))


def chunk_bytes(g):
    return int(np.prod(g["chunks"], dtype=object)) * g["elem_size"]


def array_bytes(g):
    return int(np.prod(g["shape"], dtype=object)) * g["elem_size"]


def shuffle(data, es):
    """byte j of element e to j * count + e; the len % es leftover bytes unchanged behind the planes"""
    a = np.frombuffer(bytes(data), np.uint8)
    count = len(a) // es
    return a[:count * es].reshape(count, es).T.tobytes() + a[count * es:].tobytes()


def unshuffle(data, es):
    a = np.frombuffer(bytes(data), np.uint8)
    count = len(a) // es
    return a[:count * es].reshape(es, count).T.tobytes() + a[count * es:].tobytes()


def as_elements(data, g):
    """array bytes as an ndarray of shape + (elem_size,)"""
    return np.frombuffer(bytes(data), np.uint8).reshape(tuple(g["shape"]) + (g["elem_size"],))


def random_array(g, seed):
    return np.random.default_rng(seed).integers(0, 256, array_bytes(g), dtype=np.uint8).tobytes()


def smooth_array(g, seed):
    """compressible bytes: a slow ramp with a little noise in the low byte"""
    n = array_bytes(g)
    rng = np.random.default_rng(seed)
    return ((np.arange(n) // 7 + rng.integers(0, 2, n)) & 255).astype(np.uint8).tobytes()


def region(g, c):
    """the slices of chunk c's existing elements in the array"""
    p = np.unravel_index(c, cells(g))
    return tuple(slice(int(pd) * cd, min((int(pd) + 1) * cd, sd)) for pd, cd, sd in zip(p, g["chunks"], g["shape"]))


def chunk_of(data, g, c, shuffled=None, pad=None):
    """the decoded bytes of chunk c of the array: full-sized, padded with fill (or `pad`), shuffled where the grid says so"""
    es = g["elem_size"]
    full = np.empty(tuple(g["chunks"]) + (es,), np.uint8)
    full[...] = np.frombuffer(g["fill"] if pad is None else pad, np.uint8)
    part = as_elements(data, g)[region(g, c)]
    full[tuple(slice(0, k) for k in part.shape[:-1])] = part
    raw = full.tobytes()
    return shuffle(raw, es) if (g["shuffle"] if shuffled is None else shuffled) else raw


def place(chunks, g, into=None):
    """decoded (unshuffled) chunks into an array; None: fill, the string "skip": the region keeps what `into` has"""
    es = g["elem_size"]
    out = np.frombuffer(bytes(into), np.uint8).copy().reshape(tuple(g["shape"]) + (es,)) if into is not None else np.zeros(tuple(g["shape"]) + (es,), np.uint8)
    for c, ch in enumerate(chunks):
        if isinstance(ch, str):
            continue
        r = region(g, c)
        if ch is None:
            out[r] = np.frombuffer(g["fill"], np.uint8)
        else:
            full = np.frombuffer(ch, np.uint8).reshape(tuple(g["chunks"]) + (es,))
            out[r] = full[tuple(slice(0, s.stop - s.start) for s in r)]
    return out.tobytes()


def compress(data, wrap, level=6):
    if wrap == WRAP_GZIP:
        return gzip.compress(data, compresslevel=level, mtime=0)
    o = zlib.compressobj(level, zlib.DEFLATED, 15 if wrap == WRAP_ZLIB else -15)
    return o.compress(data) + o.flush()


def decompress(data, wrap):
    """(bytes, unused tail length)"""
    o = zlib.decompressobj({WRAP_ZLIB: 15, WRAP_RAW: -15, WRAP_GZIP: 31}[wrap])
    out = o.decompress(data)
    assert o.eof
    return out, len(o.unused_data)


def encoded_chunks(data, g, level=6, pad=None):
    """every chunk of the array as its writer would store it"""
    return [compress(chunk_of(data, g, c, pad=pad), g["wrap"], level) for c in range(n_chunks(g))]


# ---- the failing variants of a chunk whose decoded bytes are `raw`; each (name, bytes, flags, code, message or None)
def failing_chunks(raw, g):
    es, wrap = g["elem_size"], g["wrap"]
    good = compress(raw, wrap)
    out = []
    body = bytearray(compress(raw, wrap, 0))  # stored blocks: a flipped LEN word is an error whatever the bytes are
    head = {WRAP_ZLIB: 2, WRAP_RAW: 0, WRAP_GZIP: 10}[wrap]
    body[head + 1] ^= 0x55
    out.append(("corrupted body", bytes(body), 0, ZS_DATA_ERROR, "invalid stored block lengths"))
    if wrap == WRAP_ZLIB:
        bad = bytearray(good)
        bad[-1] ^= 1
        out.append(("wrong Adler-32", bytes(bad), 0, ZS_DATA_ERROR, "incorrect data check"))
    if wrap == WRAP_GZIP:
        bad = bytearray(good)
        bad[-5] ^= 1
        out.append(("wrong CRC-32", bytes(bad), 0, ZS_DATA_ERROR, "incorrect data check"))
    out.append(("a stream of chunk_bytes - elem_size", compress(raw[:-es], wrap), 0, ZS_DATA_ERROR, "incorrect chunk length"))
    out.append(("a stream of chunk_bytes + elem_size", compress(raw + raw[:es], wrap), 0, ZS_BUF_ERROR, "buffer error"))
    out.append(("a STORED chunk one byte short", raw[:-1], STORED, ZS_DATA_ERROR, "incorrect chunk length"))
    out.append(("a stream cut in half", good[:len(good) // 2], 0, ZS_BUF_ERROR, "buffer error"))
    return out


# ---- the shapes: ranks 1..4, every axis 1 below, on and 1 above a chunk multiple
def edge_grids(elem_size, shuffle=True, wrap=WRAP_ZLIB, fill=None):
    chunks = {1: (24,), 2: (5, 17), 3: (3, 4, 9), 4: (2, 3, 2, 7)}
    out = []
    for rank, ch in chunks.items():
        for delta in (-1, 0, 1):
            shape = tuple(2 * c + delta for c in ch)
            out.append(grid(shape, ch, elem_size, shuffle, wrap, fill))
    return out


def zarray(shape, chunks, dtype="<f4", compressor={"id": "zlib", "level": 6}, filters=None, fill_value=0, order="C", zarr_format=2, **more):
    d = {"zarr_format": zarr_format, "shape": list(shape), "chunks": list(chunks), "dtype": dtype, "compressor": compressor, "fill_value": fill_value,
         "order": order, "filters": filters}
    d.update(more)
    return d
