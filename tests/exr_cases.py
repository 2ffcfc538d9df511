"""OpenEXR files for the tests, written field by field from the rules in include/zsgpu.h (not from zs_exr.h), and a reader
model with zlib and numpy.  A channel plane is a numpy array of H x W unsigned integers of the sample's size ("<u2" for HALF,
"<u4" for UINT and FLOAT): the library moves bytes, so the tests compare bytes.

build() has a knob for every rule: magic, version word, long names, any attribute replaced, removed or added, channel fields,
compression, the windows, line order, tiles and their mode, chunks stored raw, junk between bodies, the bodies' order, and an
edit hook over every chunk's coordinates, size and data.  CLAIMS lists every error class beside its nearest legal file."""
import struct
import zlib

import numpy as np

MAGIC = bytes([0x76, 0x2F, 0x31, 0x01])
UINT, HALF, FLOAT = 0, 1, 2
SIZE = {UINT: 4, HALF: 2, FLOAT: 4}
ZS_DATA_ERROR, ZS_BUF_ERROR = -3, -5


def sample_bytes(t):
    return SIZE.get(t, 4)


def pixels(width, height, channels, seed=0, noise=False):
    """{name: H x W array}: smooth ramps with a little noise (they deflate well), or noise alone (they do not)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, (name, t) in enumerate(channels):
        bits = 8 * sample_bytes(t)
        if noise:
            a = rng.integers(0, 1 << bits, size=(height, width), dtype=np.uint64)
        else:
            y, x = np.mgrid[0:height, 0:width]
            a = (x * 3 + y * 5 + k * 1000 + rng.integers(0, 3, size=(height, width))).astype(np.uint64) % (1 << bits)
        out[name] = a.astype("<u%d" % (bits // 8))
    return out


# ------------------------------------------------------------------ the model of the two steps
def predict(raw):
    """raw bytes -> what is handed to zlib: the bytes at even places, then those at odd places, then differences + 128."""
    a = np.frombuffer(bytes(raw), np.uint8)
    t = np.concatenate([a[0::2], a[1::2]])
    d = t.copy()
    d[1:] = t[1:] - t[:-1] + np.uint8(128)
    return d.tobytes()


def unpredict(t):
    t = np.frombuffer(bytes(t), np.uint8)
    n = t.size
    s = np.cumsum(t, dtype=np.uint8) - (np.arange(n) * 128).astype(np.uint8)
    h = (n + 1) // 2
    raw = np.empty(n, np.uint8)
    raw[0::2] = s[:h]
    raw[1::2] = s[h:]
    return raw.tobytes()


assert predict(bytes([1, 2, 3, 4, 5])) == bytes([0x01, 0x82, 0x82, 0x7D, 0x82]) and unpredict(bytes([0x01, 0x82, 0x82, 0x7D, 0x82])) == bytes([1, 2, 3, 4, 5])


# ------------------------------------------------------------------ the output layout
def plane_layout(width, height, channels):
    """([plane_off], out_len): plane c at the running sum rounded up to 16."""
    offs, end = [], 0
    for _, t in channels:
        off = (end + 15) & ~15
        offs.append(off)
        end = off + width * height * sample_bytes(t)
    return offs, end


def pack_planes(planes, width, height, channels, fill=0):
    offs, end = plane_layout(width, height, channels)
    out = np.full(end, fill, np.uint8)
    for (name, t), off in zip(channels, offs):
        b = np.ascontiguousarray(planes[name]).view(np.uint8).reshape(-1)
        out[off:off + b.size] = b
    return out


def written_mask(width, height, channels):
    """True for the bytes of the output that belong to a plane."""
    offs, end = plane_layout(width, height, channels)
    m = np.zeros(end, bool)
    for (_, t), off in zip(channels, offs):
        m[off:off + width * height * sample_bytes(t)] = True
    return m


def chunk_raw(planes, channels, x, y, w, h):
    """for each row, for each channel in list order, w samples"""
    return b"".join(np.ascontiguousarray(planes[name][r, x:x + w]).tobytes() for r in range(y, y + h) for name, _ in channels)


# ------------------------------------------------------------------ the builder
def attr(name, kind, value):
    name = name if isinstance(name, bytes) else name.encode()
    return name + b"\0" + kind.encode() + b"\0" + struct.pack("<i", len(value)) + value


def chlist(channels, fields=None):
    out = b""
    for name, t in channels:
        plinear, xs, ys = (fields or {}).get(name, (0, 1, 1))
        out += name.encode() + b"\0" + struct.pack("<iB3xii", t, plinear, xs, ys)
    return out + b"\0"


def chunk_places(width, height, compression, tile):
    """[(coordinates, x, y, w, h)] in the offset table's order"""
    if tile:
        tw, th = tile
        nx, ny = -(-width // tw), -(-height // th)
        return [((tx, ty, 0, 0), tx * tw, ty * th, min(tw, width - tx * tw), min(th, height - ty * th)) for ty in range(ny) for tx in range(nx)]
    lines = 16 if compression == 3 else 1
    return [((y,), 0, y, width, min(lines, height - y)) for y in range(0, height, lines)]


def build(planes, width, height, channels, compression=3, x_min=0, y_min=0, line_order=0, tile=None, tile_mode=0, long_names=False, version=None, magic=MAGIC,
          attrs=None, display=True, chan_fields=None, raw_chunks=(), junk=0, body_order=None, level=6, edit=None):
    """The file.  attrs: {name: (type, value bytes) or None} replaces, removes or adds attributes.  raw_chunks: indices stored
    raw although the file is compressed.  junk: that many bytes between bodies.  body_order: the table slots in the order their
    bodies lie in the file (default: ascending, descending for line order 1).  edit(k, coords, size, data) -> (coords, size,
    data) may falsify chunk k."""
    if version is None:
        version = 2 | (0x200 if tile else 0) | (0x400 if long_names else 0)
    std = [("channels", ("chlist", chlist(channels, chan_fields))),
           ("compression", ("compression", bytes([compression]))),
           ("dataWindow", ("box2i", struct.pack("<4i", x_min, y_min, x_min + width - 1, y_min + height - 1))),
           ("displayWindow", ("box2i", struct.pack("<4i", 0, 0, width - 1, height - 1)) if display else None),
           ("lineOrder", ("lineOrder", bytes([line_order]))),
           ("pixelAspectRatio", ("float", struct.pack("<f", 1.0))),
           ("tiles", ("tiledesc", struct.pack("<IIB", tile[0], tile[1], tile_mode)) if tile else None)]
    names = [n for n, _ in std]
    head = magic + struct.pack("<I", version)
    for name, v in std + [(n, v) for n, v in (attrs or {}).items() if n not in names]:
        if attrs and name in attrs:
            v = attrs[name]
        if v is not None:
            head += attr(name, v[0], v[1])
    head += b"\0"
    places = chunk_places(width, height, compression, tile)
    bodies = []
    for k, (coords, x, y, w, h) in enumerate(places):
        raw = chunk_raw(planes, channels, x, y, w, h)
        data = raw
        if compression != 0 and k not in raw_chunks:
            z = zlib.compress(predict(raw), level)
            data = z if len(z) < len(raw) else raw
        coords = tuple(c + y_min for c in coords) if not tile else coords
        size = len(data)
        if edit:
            coords, size, data = edit(k, coords, size, data)
        bodies.append(struct.pack("<%di" % len(coords), *coords) + struct.pack("<i", size) + data)
    order = list(body_order) if body_order is not None else list(range(len(places)))[::-1 if line_order == 1 else 1]
    at = len(head) + 8 * len(places)
    table, body = [0] * len(places), b""
    for k in order:
        body += bytes([0xA5]) * junk
        table[k] = at + len(body)
        body += bodies[k]
    return head + struct.pack("<%dQ" % len(places), *table) + body


def simple(width, height, channels, seed=1, noise=False, **kw):
    """(file, planes)"""
    planes = pixels(width, height, channels, seed, noise)
    return build(planes, width, height, channels, **kw), planes


# ------------------------------------------------------------------ the reader model
def cstr(f, at):
    end = f.index(b"\0", at)
    return f[at:end], end + 1


def read(f):
    """A legal file -> (info dict, [(name, type)], the planes packed as the decode call lays them out with zeros between them,
    [chunk dicts: at (the chunk's header), off (its data), size, raw_len, x, y, w, h])."""
    f = bytes(f)
    assert f[:4] == MAGIC
    version = struct.unpack_from("<I", f, 4)[0]
    assert version & 0xFF == 2 and not version & ~0x6FF
    tiled, at, a = bool(version & 0x200), 8, {}
    while f[at]:
        name, at = cstr(f, at)
        kind, at = cstr(f, at)
        size = struct.unpack_from("<i", f, at)[0]
        a[name.decode("latin-1")] = (kind.decode(), f[at + 4:at + 4 + size])
        at += 4 + size
    at += 1
    channels, p, cl = [], 0, a["channels"][1]
    while cl[p]:
        name, p = cstr(cl, p)
        t, _, xs, ys = struct.unpack_from("<iB3xii", cl, p)
        assert t in SIZE and xs == 1 and ys == 1
        channels.append((name.decode("latin-1"), t))
        p += 16
    compression, line_order = a["compression"][1][0], a["lineOrder"][1][0]
    assert compression in (0, 2, 3)
    x0, y0, x1, y1 = struct.unpack("<4i", a["dataWindow"][1])
    width, height = x1 - x0 + 1, y1 - y0 + 1
    tile = None
    if tiled:
        tw, th, mode = struct.unpack("<IIB", a["tiles"][1])
        assert mode & 15 == 0
        tile = (tw, th)
    places = chunk_places(width, height, compression, tile)
    table = struct.unpack_from("<%dQ" % len(places), f, at)
    offs, out_len = plane_layout(width, height, channels)
    out = np.zeros(out_len, np.uint8)
    views = [out[o:o + width * height * sample_bytes(t)].reshape(height, width * sample_bytes(t)) for (_, t), o in zip(channels, offs)]
    chunks = []
    for (coords, x, y, w, h), off in zip(places, table):
        nc = len(coords)
        got = struct.unpack_from("<%di" % nc, f, off)
        assert got == (coords if tiled else (coords[0] + y0,)), (got, coords)
        size = struct.unpack_from("<i", f, off + 4 * nc)[0]
        data = f[off + 4 * nc + 4:off + 4 * nc + 4 + size]
        U = w * h * sum(sample_bytes(t) for _, t in channels)
        assert 0 <= size <= U and len(data) == size
        raw = data if size == U else unpredict(zlib.decompress(data))
        assert len(raw) == U
        p = 0
        for r in range(y, y + h):
            for (_, t), v in zip(channels, views):
                n = w * sample_bytes(t)
                v[r, x * sample_bytes(t):x * sample_bytes(t) + n] = np.frombuffer(raw[p:p + n], np.uint8)
                p += n
        chunks.append(dict(at=off, off=off + 4 * nc + 4, size=size, raw_len=U, x=x, y=y, w=w, h=h))
    info = dict(width=width, height=height, compression=compression, line_order=line_order, tiled=int(tiled), tile=tile, data_window=(x0, y0, x1, y1),
                display_window=struct.unpack("<4i", a["displayWindow"][1]) if "displayWindow" in a else None, n_chunks=len(places), out_len=out_len,
                version=version, attrs=a)
    return info, channels, out, chunks


# ------------------------------------------------------------------ every error class beside its nearest legal file
RG = [("G", HALF), ("R", HALF)]


def _claims():
    W, H = 6, 20
    planes = pixels(W, H, RG, seed=40)
    b = lambda **kw: build(planes, W, H, RG, **kw)  # noqa: E731
    box = lambda *v: ("box2i", struct.pack("<4i", *v))  # noqa: E731
    legal = b()
    head_end = legal.index(b"lineOrder")
    table_at = read(legal)[3][0]["at"] - 16
    many = lambda n: [("c%02d" % k, HALF) for k in range(n)]  # noqa: E731
    few = lambda n: build(pixels(2, 1, many(n), seed=41), 2, 1, many(n))  # noqa: E731
    one_wide = build(pixels(1, H, RG, seed=42), 1, H, RG)
    out = [
        # (what, the nearest legal file, the file with the error, its code, its message)
        ("magic", legal, b(magic=bytes([0x76, 0x2F, 0x31, 0x02])), ZS_DATA_ERROR, "not an OpenEXR file"),
        ("version 3", legal, b(version=3), ZS_DATA_ERROR, "unsupported file version"),
        ("deep", b(version=2 | 0x400), b(version=2 | 0x800), ZS_DATA_ERROR, "deep data is not supported"),
        ("multi-part", b(version=2 | 0x400), b(version=2 | 0x1000), ZS_DATA_ERROR, "multi-part files are not supported"),
        ("flag bits", b(version=2 | 0x400), b(version=2 | 0x2000), ZS_DATA_ERROR, "unsupported version flags"),
        ("flag bit 0x100", b(version=2 | 0x400), b(version=2 | 0x100), ZS_DATA_ERROR, "unsupported version flags"),
        ("header cut", legal, legal[:head_end + 3], ZS_DATA_ERROR, "the header reaches out of the file"),
        ("attribute larger than the file", b(attrs={"x": ("string", b"abc")}), b(attrs={"x": ("string", b"abc")}).replace(b"x\0string\0\x03\0\0\0", b"x\0string\0\xff\xff\xff\x7f"),
         ZS_DATA_ERROR, "the header reaches out of the file"),
        ("name of 32", b(attrs={"n" * 31: ("string", b"abc")}), b(attrs={"n" * 32: ("string", b"abc")}), ZS_DATA_ERROR, "a name is longer than the version flags allow"),
        ("long name of 256", b(long_names=True, attrs={"n" * 255: ("string", b"abc")}), b(long_names=True, attrs={"n" * 256: ("string", b"abc")}), ZS_DATA_ERROR,
         "a name is longer than the version flags allow"),
        ("compression of 2 bytes", legal, b(attrs={"compression": ("compression", b"\3\0")}), ZS_DATA_ERROR, "an attribute's size disagrees with its type"),
        ("dataWindow of 12 bytes", legal, b(attrs={"dataWindow": ("box2i", b"\0" * 12)}), ZS_DATA_ERROR, "an attribute's size disagrees with its type"),
        ("lineOrder as int", legal, b(attrs={"lineOrder": ("int", b"\0\0\0\0")}), ZS_DATA_ERROR, "an attribute's size disagrees with its type"),
        ("channels as string", legal, b(attrs={"channels": ("string", chlist(RG))}), ZS_DATA_ERROR, "an attribute's size disagrees with its type"),
        ("tiles of 8 bytes", b(tile=(4, 4)), b(tile=(4, 4), attrs={"tiles": ("tiledesc", b"\4\0\0\0\4\0\0\0")}), ZS_DATA_ERROR, "an attribute's size disagrees with its type"),
        ("window inverted in x", one_wide, b(attrs={"dataWindow": box(4, 0, 3, H - 1)}), ZS_DATA_ERROR, "invalid data window"),
        ("window inverted in y", legal, b(attrs={"dataWindow": box(0, 7, W - 1, 6)}), ZS_DATA_ERROR, "invalid data window"),
        ("no channels", few(1), b(attrs={"channels": ("chlist", b"\0")}), ZS_DATA_ERROR, "no channels"),
        ("65 channels", few(64), few(65), ZS_DATA_ERROR, "more than 64 channels"),
        ("pixel type 3", legal, build(planes, W, H, [("G", 3), ("R", HALF)]), ZS_DATA_ERROR, "unsupported pixel type"),
        ("x sampling 2", b(chan_fields={"G": (1, 1, 1)}), b(chan_fields={"G": (0, 2, 1)}), ZS_DATA_ERROR, "unsupported channel sampling"),
        ("y sampling 2", b(chan_fields={"R": (1, 1, 1)}), b(chan_fields={"R": (0, 1, 2)}), ZS_DATA_ERROR, "unsupported channel sampling"),
        ("mipmap", b(tile=(4, 4), tile_mode=0x10), b(tile=(4, 4), tile_mode=1), ZS_DATA_ERROR, "unsupported level mode"),
        ("ripmap", b(tile=(4, 4), tile_mode=0x10), b(tile=(4, 4), tile_mode=2), ZS_DATA_ERROR, "unsupported level mode"),
        ("tile width 0", b(tile=(4, 4)), b(tile=(4, 4), attrs={"tiles": ("tiledesc", struct.pack("<IIB", 0, 4, 0))}), ZS_DATA_ERROR, "invalid tile size"),
        ("tile height 0", b(tile=(4, 4)), b(tile=(4, 4), attrs={"tiles": ("tiledesc", struct.pack("<IIB", 4, 0, 0))}), ZS_DATA_ERROR, "invalid tile size"),
        ("random order on scanlines", b(tile=(4, 4), line_order=2), b(line_order=2, body_order=range(2)), ZS_DATA_ERROR, "random line order in a scanline file"),
        ("table cut", legal[:table_at + 16], legal[:table_at + 15], ZS_DATA_ERROR, "the offset table reaches out of the file"),
        ("too large", legal, b(attrs={"dataWindow": box(0, 0, 32767, 32767)}), ZS_DATA_ERROR, "the image is above 2 GiB - 1 KiB"),
        ("shorter than 8", legal, legal[:7], ZS_BUF_ERROR, "buffer error"),
    ]
    for name in ("channels", "compression", "dataWindow", "lineOrder"):
        out.append(("no " + name, legal, b(attrs={name: None}), ZS_DATA_ERROR, "a required attribute is missing"))
    out.append(("no tiles", b(tile=(4, 4)), b(tile=(4, 4), attrs={"tiles": None}), ZS_DATA_ERROR, "a required attribute is missing"))
    for k, comp in enumerate((1, 4, 5, 6, 7, 8, 9)):
        out.append(("compression %d" % comp, b(compression=(0, 2, 3)[k % 3]), b(attrs={"compression": ("compression", bytes([comp]))}), ZS_DATA_ERROR,
                    "unsupported compression method"))
    return out


CLAIMS = _claims()

# per chunk: (what, edit hook for chunk 1 of three, the chunk's code, its message)
CHUNK_CLAIMS = [
    ("wrong y", lambda k, c, n, d: ((c[0] + 1,), n, d) if k == 1 else (c, n, d), ZS_DATA_ERROR, "a chunk's coordinates do not match its place"),
    ("size above U", lambda k, c, n, d: (c, 16 * 6 * 4 + 1, d + b"\0" * 400) if k == 1 else (c, n, d), ZS_DATA_ERROR, "invalid chunk size"),
    ("negative size", lambda k, c, n, d: (c, -1, d) if k == 1 else (c, n, d), ZS_DATA_ERROR, "invalid chunk size"),
]
