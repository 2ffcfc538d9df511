"""TIFF files for the TIFF tests, none of them read by the library under test before a test hands them over: a seeded pixel
generator, the two predictors in numpy, a field-by-field builder (byte order, classic or BigTIFF, strips or tiles, predictor,
compression 1 / 8 / 32946, a padded or a short last strip, more pages, chunks at odd offsets, any tag replaced or removed),
and a pure-Python reader (IFD walk, zlib.decompress, numpy unpredict) for the files the library writes.

Pixels are always handled as `rows`: a uint8 array of shape (height, row_bytes) holding the image exactly as the decode call
leaves it and the encode call takes it -- rows of ceil(width * spp * bits / 8) bytes, samples little-endian."""
import struct
import zlib

import numpy as np

DTYPES = {8: "u1", 16: "u2", 32: "u4"}
TYPE_BYTES = {1: 1, 3: 2, 4: 4, 16: 8}
TYPE_CODES = {1: "B", 3: "H", 4: "I", 16: "Q"}


def row_bytes(width, spp, bits):
    return (width * spp * bits + 7) // 8


def pixels(width, height, spp=1, bits=8, seed=0, fmt=1):
    """Seeded rows: smooth ramps with a little noise (so that the predictor matters and deflate has something to do); floats
    (fmt 3) lie in [0, 1) and hold subnormals, zeros and negative values too."""
    rng = np.random.default_rng([seed, width, height, spp, bits, fmt])
    if bits < 8:
        return rng.integers(0, 256, (height, row_bytes(width, spp, bits)), dtype=np.uint8)
    y, x, c = np.meshgrid(np.arange(height), np.arange(width), np.arange(spp), indexing="ij")
    if fmt == 3:
        v = (np.sin(x / 9.0 + c) * np.cos(y / 7.0) * 0.5 + rng.random((height, width, spp)) * 1e-3).astype("<f4")
        v.reshape(-1)[::17] = 0
        v.reshape(-1)[5::31] = np.float32(1e-41)
        return v.view(np.uint8).reshape(height, -1)
    top = (1 << bits) - 1
    v = (x * 3 + y * 5 + c * 40 + rng.integers(0, 4, (height, width, spp))) * (top // 255 if bits > 8 else 1) % (top + 1)
    return v.astype("<" + DTYPES[bits]).view(np.uint8).reshape(height, -1)


def all_ff_differences(width, height, spp, bits):
    """Rows whose horizontal differences are all ones in every bit: every sum carries through all of a sample's bytes."""
    top = 1 << bits
    x = np.arange(1, width + 1, dtype=np.uint64)[None, :, None] * np.uint64(top - 1) % np.uint64(top)
    v = np.broadcast_to(x, (height, width, spp))
    return np.ascontiguousarray(v.astype("<" + DTYPES[bits])).view(np.uint8).reshape(height, -1)


# ---- the predictors, on one chunk given as rows of little-endian samples: (rows, chunk_w * spp * bits / 8) uint8
def predict(chunk, spp, bits, predictor, order="<"):
    """The chunk's bytes as they are deflated: differenced (2) or plane-split and differenced (3), samples in `order`."""
    n = chunk.shape[0]
    if bits < 8 or (predictor == 1 and (bits == 8 or order == "<")):
        return np.ascontiguousarray(chunk)
    if predictor == 3:
        be = chunk.reshape(n, -1, 4)[:, :, ::-1]  # the most significant byte first
        planes = np.ascontiguousarray(be.transpose(0, 2, 1)).reshape(n, -1)
        out = planes.copy()
        out[:, spp:] -= planes[:, :-spp]
        return out
    v = chunk.view("<" + DTYPES[bits]).reshape(n, -1, spp)
    if predictor == 2:
        d = v.copy()
        d[:, 1:] -= v[:, :-1]
        v = d
    return np.ascontiguousarray(v.astype(order + DTYPES[bits])).view(np.uint8).reshape(n, -1)


def unpredict(data, spp, bits, predictor, order="<"):
    """The inverse: a decoded chunk's bytes (rows, bytes) -> rows of little-endian samples."""
    n = data.shape[0]
    if bits < 8 or (predictor == 1 and (bits == 8 or order == "<")):
        return np.ascontiguousarray(data)
    if predictor == 3:
        acc = np.cumsum(data.reshape(n, -1, spp), axis=1, dtype=np.uint8).reshape(n, 4, -1)
        return np.ascontiguousarray(acc.transpose(0, 2, 1)[:, :, ::-1]).reshape(n, -1)
    v = data.view(order + DTYPES[bits]).reshape(n, -1, spp).astype("<" + DTYPES[bits])
    if predictor == 2:
        v = np.cumsum(v, axis=1, dtype=v.dtype)
    return np.ascontiguousarray(v).view(np.uint8).reshape(n, -1)


def cut(rows, width, spp, bits, x, y, cw, ch, pad_rows=True):
    """The chunk of cw x ch pixels at (x, y) of the image: its surplus columns, and with pad_rows its surplus rows, repeat the
    last pixel and the last row (below 8 bits the surplus columns are zero)."""
    h = rows.shape[0]
    part = rows[y:y + ch]
    if bits < 8:
        b0, nb = x * spp * bits // 8, row_bytes(cw, spp, bits)
        part = part[:, b0:b0 + nb]
        part = np.pad(part, ((0, 0), (0, nb - part.shape[1])))
    else:
        px = spp * bits // 8
        part = part.reshape(part.shape[0], width, px)[:, x:x + cw]
        part = np.pad(part, ((0, 0), (0, cw - part.shape[1]), (0, 0)), mode="edge").reshape(part.shape[0], cw * px)
    if pad_rows and part.shape[0] < ch:
        part = np.pad(part, ((0, ch - part.shape[0]), (0, 0)), mode="edge")
    return np.ascontiguousarray(part)


def chunk_grid(width, height, cw, ch):
    return [(x, y) for y in range(0, height, ch) for x in range(0, width, cw)]


# ---- the builder
def page(rows, width, spp=1, bits=8, fmt=1, predictor=1, compression=8, tile=None, rows_per_strip=None, pad_last_strip=False, order="<", level=6,
         photometric=None, extra=None, tags=None, chunk_edit=None):
    """One page: (entries, chunk bodies).  entries: {tag: (type, [values])}, the offsets' entry filled by build().  tags: entries
    to replace ({tag: (type, values)}) or remove ({tag: None}); chunk_edit(k, body) -> body replaces chunk k's bytes."""
    height = rows.shape[0]
    cw, ch = tile if tile else (width, min(rows_per_strip or height, height))
    bodies = []
    for k, (x, y) in enumerate(chunk_grid(width, height, cw, ch)):
        c = cut(rows, width, spp, bits, x, y, cw, ch, pad_rows=bool(tile) or pad_last_strip)
        raw = predict(c, spp, bits, predictor, order).tobytes()
        body = raw if compression == 1 else zlib.compress(raw, level)
        bodies.append(chunk_edit(k, body) if chunk_edit else body)
    if photometric is None:
        photometric = 2 if spp >= 3 else 1
    e = {256: (4, [width]), 257: (4, [height]), 258: (3, [bits] * spp), 259: (3, [compression]), 262: (3, [photometric]), 277: (3, [spp]),
         284: (3, [1]), 339: (3, [fmt] * spp)}
    if predictor != 1:
        e[317] = (3, [predictor])
    if tile:
        e[322], e[323], e[324], e[325] = (3, [cw]), (3, [ch]), (4, None), (4, [len(b) for b in bodies])
    else:
        e[273], e[279] = (4, None), (4, [len(b) for b in bodies])
        if rows_per_strip is not None:
            e[278] = (3 if rows_per_strip < 65536 else 4, [rows_per_strip])
    if extra:
        e[338] = (3, list(extra))
    for tag, v in (tags or {}).items():
        if v is None:
            e.pop(tag, None)
        else:
            e[tag] = v
    return e, bodies


def build(pages, order="<", big=False, odd_offsets=False, loop=False):
    """A file of these pages (page() results): [header | per page: IFD, its longer values | the chunks of all pages].  BigTIFF
    writes offsets and byte counts as LONG8.  odd_offsets: every chunk begins at an odd offset.  loop: the last IFD points
    back at the first."""
    head, each, tail, inline = (8, 20, 8, 8) if big else (2, 12, 4, 4)
    word = "Q" if big else "I"
    pages = [(dict(e), b) for e, b in pages]
    if big:
        for e, _ in pages:
            for tag in (273, 279, 324, 325):
                if tag in e and e[tag][0] == 4:
                    e[tag] = (16, e[tag][1])
    at = 16 if big else 8
    ifd_at, val_at = [], []
    for e, bodies in pages:
        ifd_at.append(at)
        at += head + each * len(e) + tail
        val_at.append(at)
        for tag, (typ, vals) in e.items():
            n = TYPE_BYTES[typ] * (len(bodies) if vals is None else len(vals))
            if n > inline:
                at += n + (n & 1)
    out = bytearray(at)
    out[:4] = (b"II" if order == "<" else b"MM") + struct.pack(order + "H", 43 if big else 42)
    if big:
        out[4:16] = struct.pack(order + "HHQ", 8, 0, ifd_at[0])
    else:
        out[4:8] = struct.pack(order + "I", ifd_at[0])
    for k, (e, bodies) in enumerate(pages):
        offs = []
        for b in bodies:
            if (len(out) & 1) != (1 if odd_offsets else 0):
                out += b"\0"
            offs.append(len(out))
            out += b
        for tag in (273, 324):
            if tag in e and e[tag][1] is None:
                e[tag] = (e[tag][0], offs)
        p, v = ifd_at[k], val_at[k]
        struct.pack_into(order + ("Q" if big else "H"), out, p, len(e))
        p += head
        for tag in sorted(e):
            typ, vals = e[tag]
            data = struct.pack(order + TYPE_CODES[typ] * len(vals), *vals)
            struct.pack_into(order + "HH" + word, out, p, tag, typ, len(vals))
            if len(data) <= inline:
                out[p + each - inline:p + each - inline + len(data)] = data
            else:
                struct.pack_into(order + word, out, p + each - inline, v)
                out[v:v + len(data)] = data
                v += len(data) + (len(data) & 1)
            p += each
        nxt = ifd_at[k + 1] if k + 1 < len(pages) else (ifd_at[0] if loop else 0)
        struct.pack_into(order + word, out, p, nxt)
    return bytes(out)


def simple(rows, width, spp=1, bits=8, order="<", big=False, odd_offsets=False, **kw):
    """One page, one call."""
    return build([page(rows, width, spp, bits, order=order, **kw)], order=order, big=big, odd_offsets=odd_offsets)


# ---- the reader
class TiffError(Exception):
    pass


def read_ifds(data):
    """[{tag: [values]}] of the chain, and the byte order."""
    if len(data) < 8 or data[:2] not in (b"II", b"MM"):
        raise TiffError("header")
    order = "<" if data[:2] == b"II" else ">"
    version, = struct.unpack_from(order + "H", data, 2)
    big = version == 43
    if version not in (42, 43):
        raise TiffError("version")
    at, = struct.unpack_from(order + ("Q" if big else "I"), data, 8 if big else 4)
    head, each, inline, word = (8, 20, 8, "Q") if big else (2, 12, 4, "I")
    ifds, seen = [], set()
    while at:
        if at in seen:
            raise TiffError("loop")
        seen.add(at)
        n, = struct.unpack_from(order + ("Q" if big else "H"), data, at)
        tags = {}
        for k in range(n):
            p = at + head + each * k
            tag, typ, count = struct.unpack_from(order + "HH" + word, data, p)
            if typ in TYPE_BYTES:
                size = TYPE_BYTES[typ] * count
                where = p + each - inline if size <= inline else struct.unpack_from(order + word, data, p + each - inline)[0]
                tags[tag] = list(struct.unpack_from(order + TYPE_CODES[typ] * count, data, where))
        ifds.append(tags)
        at, = struct.unpack_from(order + word, data, at + head + each * n)
    return ifds, order


def read(data, page_index=0):
    """(tags, rows) of one page: the pixels as the decode call must leave them."""
    ifds, order = read_ifds(data)
    t = ifds[page_index]
    width, height, spp = t[256][0], t[257][0], t.get(277, [1])[0]
    bits, predictor, compression = t.get(258, [1])[0], t.get(317, [1])[0], t.get(259, [1])[0]
    tiled = 322 in t
    cw, ch = (t[322][0], t[323][0]) if tiled else (width, min(t.get(278, [height])[0], height))
    offs, lens = (t[324], t[325]) if tiled else (t[273], t[279])
    rb, crb = row_bytes(width, spp, bits), row_bytes(cw, spp, bits)
    rows = np.zeros((height, rb), np.uint8)
    grid = chunk_grid(width, height, cw, ch)
    assert len(grid) == len(offs) == len(lens)
    for (x, y), off, n in zip(grid, offs, lens):
        body = data[off:off + n]
        assert len(body) == n
        raw = body if compression == 1 else zlib.decompress(body)
        h = min(ch, height - y)
        assert len(raw) >= (ch if tiled else h) * crb
        px = unpredict(np.frombuffer(raw, np.uint8)[:h * crb].reshape(h, crb), spp, bits, predictor, order)
        b0 = x * spp * bits // 8
        keep = min(rb - b0, crb)
        rows[y:y + h, b0:b0 + keep] = px[:, :keep]
    return t, rows


# ---- the golden files (tests/golden/tiff): written once by Pillow's libtiff from pixels(), see __main__
GOLDEN = [  # name, Pillow mode, width, height, spp, bits, fmt, predictor, extra Pillow arguments
    ("l_p1", "L", 97, 61, 1, 8, 1, 1, {}), ("l_p2", "L", 97, 61, 1, 8, 1, 2, {}),
    ("la_p1", "LA", 65, 40, 2, 8, 1, 1, {}), ("la_p2", "LA", 65, 40, 2, 8, 1, 2, {}),
    ("rgb_p1", "RGB", 83, 47, 3, 8, 1, 1, {}), ("rgb_p2", "RGB", 83, 47, 3, 8, 1, 2, {}),
    ("rgba_p1", "RGBA", 70, 33, 4, 8, 1, 1, {}), ("rgba_p2", "RGBA", 70, 33, 4, 8, 1, 2, {}),
    ("i16_p1", "I;16", 75, 50, 1, 16, 1, 1, {}), ("i16_p2", "I;16", 75, 50, 1, 16, 1, 2, {}),
    ("f_p1", "F", 61, 43, 1, 32, 3, 1, {}), ("f_p3", "F", 61, 43, 1, 32, 3, 3, {}),
    ("bilevel", "1", 101, 37, 1, 1, 1, 1, {}),
]


def golden_rows(name):
    """The pixels a golden file was written from.  A bilevel file's padding bits in a row's last byte are zero."""
    _, _, w, h, spp, bits, fmt, _, _ = next(g for g in GOLDEN if g[0] == name)
    rows = pixels(w, h, spp, bits, seed=1234, fmt=fmt)
    if bits == 1 and w % 8:
        rows[:, -1] &= (0xFF << (8 - w % 8)) & 0xFF
    return rows


def golden_dims(name):
    return next(g for g in GOLDEN if g[0] == name)[2:8]


if __name__ == "__main__":  # python tests/tiff_cases.py <directory>: writes the golden files (needs Pillow with libtiff)
    import os
    import sys

    from PIL import Image

    for name, mode, w, h, spp, bits, fmt, predictor, kw in GOLDEN:
        rows = golden_rows(name)
        if mode == "1":
            im = Image.frombytes("1", (w, h), rows.tobytes())
        elif mode == "F":
            im = Image.frombytes("F", (w, h), rows.tobytes())
        elif mode == "I;16":
            im = Image.frombytes("I;16", (w, h), rows.tobytes())
        else:
            im = Image.frombytes(mode, (w, h), rows.tobytes())
        tiffinfo = {317: predictor} if predictor != 1 else {}
        im.save(os.path.join(sys.argv[1], name + ".tif"), compression="tiff_adobe_deflate", tiffinfo=tiffinfo, **kw)
