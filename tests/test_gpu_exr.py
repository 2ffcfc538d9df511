"""OpenEXR files on the device, both directions (include/zsgpu.h zs_exr_*).  Ground truth is always the numpy planes a file
was built from and the model of tests/exr_cases.py (zlib and numpy), which is written from the rules in the header, not from
the library; no third-party reader was at hand.  The predictor kernels are held against the model alone first: lengths around
a 16-byte group and around a tile (32 KiB of output), three tiles plus one byte, stored bytes of all 0xFF, inputs and outputs
at odd addresses between guard bytes.  Images are at most ~1100 pixels wide and 53 high."""
import struct
import zlib

import numpy as np
import pytest

import exr_cases as xc
from zlibstream_amd import deflate_bound, exr_bound, exr_decode_files, exr_encode, exr_file_info, exr_predict, exr_unpredict

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xEE
ZS_DATA_ERROR, ZS_BUF_ERROR = -3, -5
TILE = 32 << 10  # output bytes of one tile of the kernel
RGBA = [("A", xc.HALF), ("B", xc.HALF), ("G", xc.HALF), ("R", xc.HALF)]
MIXED = [("A", xc.HALF), ("B", xc.HALF), ("G", xc.HALF), ("R", xc.HALF), ("Z", xc.FLOAT), ("id", xc.UINT)]


class Arena:
    """Device buffers at odd addresses between guard bytes: ptr(k) is buffer k's address, fill() uploads into it, results()
    returns every buffer's bytes and fails on a byte changed anywhere else."""

    def __init__(self, sizes):
        import torch
        self.off, at = [], GUARD + 1
        for n in sizes:
            self.off.append(at)
            at = (at + n + GUARD) | 1
        self.sizes = list(sizes)
        self.buf = torch.full((at + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def ptr(self, k):
        return self.buf.data_ptr() + self.off[k]

    def fill(self, k, data):
        import torch
        a = np.frombuffer(bytes(data), np.uint8)
        if a.size:
            self.buf[self.off[k]:self.off[k] + a.size] = torch.from_numpy(a.copy()).cuda()

    def results(self, written=None):
        """The buffers' bytes; `written[k]`: how many of buffer k's bytes may have changed (default: all of it)."""
        import torch
        torch.cuda.synchronize()
        got = self.buf.cpu().numpy()
        outside = got != FILL
        for k, (o, n) in enumerate(zip(self.off, self.sizes)):
            outside[o:o + (n if written is None else written[k])] = False
        assert not outside.any(), "bytes changed outside the outputs, first at %d" % int(np.flatnonzero(outside)[0])
        return [got[o:o + n] for o, n in zip(self.off, self.sizes)]


# ------------------------------------------------------------------ the predictor kernels alone
LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, TILE - 1, TILE, TILE + 1, TILE + 2, 2 * TILE - 1, 2 * TILE + 33, 3 * TILE + 1]


def kernel_cases():
    """Stored bytes: noise of every length, and all 0xFF -- every sum wraps -- at the lengths where the halves' parities differ."""
    rng = np.random.default_rng(60)
    out = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LENGTHS]
    out += [b"\xff" * n for n in (1, 2, 3, 33, 2049, TILE + 1, TILE + 2, 3 * TILE + 1)]
    return out


def run_kernel(engine, fn, data):
    src, dst = Arena([len(d) for d in data]), Arena([len(d) for d in data])
    for k, d in enumerate(data):
        src.fill(k, d)
    n = len(data)
    fn(engine, [src.ptr(k) for k in range(n)], [dst.ptr(k) for k in range(n)], [len(d) for d in data])
    src.results()  # (the inputs' guards too)
    return [g.tobytes() for g in dst.results()]


def test_undo_kernel_against_the_model(engine):
    stored = kernel_cases()
    for k, (got, t) in enumerate(zip(run_kernel(engine, exr_unpredict, stored), stored)):
        assert got == xc.unpredict(t), "case %d: %d bytes" % (k, len(t))


def test_forward_kernel_against_the_model_and_back(engine):
    raw = kernel_cases()
    mid = run_kernel(engine, exr_predict, raw)
    for k, (got, r) in enumerate(zip(mid, raw)):
        assert got == xc.predict(r), "case %d: %d bytes" % (k, len(r))
    for k, (got, r) in enumerate(zip(run_kernel(engine, exr_unpredict, mid), raw)):
        assert got == r, "case %d: %d bytes" % (k, len(r))


def test_the_worked_example_on_the_device(engine):
    assert run_kernel(engine, exr_predict, [bytes([1, 2, 3, 4, 5])]) == [bytes([0x01, 0x82, 0x82, 0x7D, 0x82])]
    assert run_kernel(engine, exr_unpredict, [bytes([0x01, 0x82, 0x82, 0x7D, 0x82])]) == [bytes([1, 2, 3, 4, 5])]


def test_kernel_calls_refuse_lengths_out_of_range(engine):
    a = Arena([16, 16])
    for n in (0, -1, 1 << 31):
        with pytest.raises(ValueError):
            exr_unpredict(engine, [a.ptr(0)], [a.ptr(1)], [n])
        with pytest.raises(ValueError):
            exr_predict(engine, [a.ptr(0)], [a.ptr(1)], [n])
    with pytest.raises(ValueError):
        exr_predict(engine, [0], [a.ptr(1)], [4])
    a.results([0, 0])


# ------------------------------------------------------------------ decode
def run_decode(engine, files, caps=None):
    """zs_exr_decode_files_batch with every output at an odd address between guard bytes.  caps: None for each file's out_len.
    Returns (code, out_len[], chunk codes[][], status[], the outputs)."""
    if caps is None:
        caps = [exr_file_info(f)[0]["out_len"] for f in files]
    out = Arena(caps)
    rc, lens, codes, status = exr_decode_files(engine, files, [out.ptr(k) for k in range(len(files))], list(caps))
    return rc, lens, codes, status, out.results()


def expect(planes, width, height, channels):
    """the output buffer: the planes, and the fill between them, which is never written"""
    return xc.pack_planes(planes, width, height, channels, fill=FILL)


def file_cases():
    """(what, file, expected output)"""
    out = []

    def add(what, width, height, channels, seed, planes=None, **kw):
        planes = planes if planes is not None else xc.pixels(width, height, channels, seed)
        out.append((what, xc.build(planes, width, height, channels, **kw), expect(planes, width, height, channels)))

    add("1 x 1", 1, 1, RGBA, 70)
    add("1 x 1 of one half", 1, 1, [("Y", xc.HALF)], 71)
    add("W = 1", 1, 40, RGBA, 72)
    for h in (15, 16, 17, 33):
        add("H = %d" % h, 21, h, RGBA, 73)
    add("ZIPS", 37, 9, MIXED, 74, compression=2)
    add("none", 37, 9, MIXED, 75, compression=0)
    add("mixed types", 37, 53, MIXED, 76)
    add("A B G R Z", 23, 18, RGBA + [("Z", xc.FLOAT)], 77)
    # 16 rows x 1100 x 8 bytes = 140800 bytes: a chunk of more than four tiles, and a last chunk of four rows
    add("wide", 1100, 20, RGBA, 78)
    add("negative origin", 30, 20, RGBA, 79, x_min=-100, y_min=-7)
    add("decreasing y", 30, 53, RGBA, 80, line_order=1)
    add("shuffled bodies and junk", 30, 53, RGBA, 81, body_order=(2, 0, 3, 1), junk=7)
    # a noise chunk between two that deflate: the builder stores it raw, as a writer does
    planes = xc.pixels(40, 48, RGBA, 82)
    noise = xc.pixels(40, 16, RGBA, 83, noise=True)
    for name, _ in RGBA:
        planes[name][16:32] = noise[name]
    add("raw between compressed", 40, 48, RGBA, 0, planes=planes)
    add("tiles 16 x 16", 37, 53, MIXED, 84, tile=(16, 16))
    add("tiles 32 x 8", 37, 53, RGBA, 85, tile=(32, 8), line_order=2, body_order=[(k * 5) % 14 for k in range(14)])
    add("tiles, none", 37, 53, RGBA, 86, tile=(16, 16), compression=0)
    add("one tile larger than the image", 5, 5, RGBA, 87, tile=(16, 16))
    add("long names", 9, 9, [("a" * 200, xc.HALF), ("b", xc.UINT)], 88, long_names=True)
    return out


def test_decode_files_against_the_model(engine):
    cases = file_cases()
    raw = next(f for what, f, _ in cases if what == "raw between compressed")
    sizes = [(c["data_len"], c["raw_len"]) for c in exr_file_info(raw)[2]]
    assert sizes[1][0] == sizes[1][1] and sizes[0][0] < sizes[0][1] and sizes[2][0] < sizes[2][1]
    wide = next(f for what, f, _ in cases if what == "wide")
    assert exr_file_info(wide)[2][0]["raw_len"] > 4 * TILE
    assert exr_file_info(cases[-3][1])[2][-1]["w"] == 5  # the corner tile of 5 x 5
    for what, f, want in cases:
        assert np.array_equal(np.where(xc.written_mask(*shape_of(f)), xc.read(f)[2], FILL), want), what  # the model agrees with the builder
    # one by one, so that a failure names its case, and then all in one call
    for what, f, want in cases:
        rc, lens, codes, status, outs = run_decode(engine, [f])
        assert rc == 0 and status == [0] and lens == [want.size] and set(codes[0]) == {0}, (what, engine.last_error())
        assert np.array_equal(outs[0], want), what
    rc, lens, codes, status, outs = run_decode(engine, [f for _, f, _ in cases])
    assert rc == 0 and status == [0] * len(cases), engine.last_error()
    for (what, _, want), got in zip(cases, outs):
        assert np.array_equal(got, want), what


def shape_of(f):
    info, channels, _, _ = xc.read(f)
    return info["width"], info["height"], channels


def test_eight_files_of_different_shapes_in_one_call(engine):
    cases = [c for c in file_cases() if c[0] in ("1 x 1", "W = 1", "H = 17", "ZIPS", "mixed types", "wide", "decreasing y", "tiles 16 x 16")]
    assert len(cases) == 8
    rc, lens, codes, status, outs = run_decode(engine, [f for _, f, _ in cases][::-1])
    assert rc == 0 and status == [0] * 8
    for (what, _, want), got in zip(cases[::-1], outs):
        assert np.array_equal(got, want), what


# ------------------------------------------------------------------ failures: each between two whole neighbours
W, H = 30, 40  # three chunks of 16, 16 and 8 rows


def neighbours():
    planes = xc.pixels(W, H, RGBA, 90)
    return planes, xc.build(planes, W, H, RGBA), expect(planes, W, H, RGBA)


def chunk_mask(y, h):
    """True for the output bytes of rows [y, y + h)"""
    offs, end = xc.plane_layout(W, H, RGBA)
    m = np.zeros(end, bool)
    for (_, t), off in zip(RGBA, offs):
        row = W * xc.SIZE[t]
        m[off + y * row:off + (y + h) * row] = True
    return m


def chunk_fails_alone(engine, bad, chunk, code, message):
    planes, good, want = neighbours()
    rc, lens, codes, status, outs = run_decode(engine, [good, bad, good])
    assert rc == code and status == [0, code, 0] and lens == [want.size] * 3
    assert engine.last_error() == "file 1: chunk %d: %s" % (chunk, message)
    expected = [0, 0, 0]
    expected[chunk] = code
    assert codes == [[0, 0, 0], expected, [0, 0, 0]]
    assert np.array_equal(outs[0], want) and np.array_equal(outs[2], want)
    keep = ~chunk_mask(16 * chunk, min(16, H - 16 * chunk))
    assert np.array_equal(outs[1][keep], want[keep])  # every other plane byte, and the fill between the planes


def edit_chunk_1(change):
    planes, _, _ = neighbours()
    return xc.build(planes, W, H, RGBA, edit=lambda k, c, n, d: change(c, n, d) if k == 1 else (c, n, d))


def test_a_flipped_adler_fails_its_chunk_alone(engine):
    bad = edit_chunk_1(lambda c, n, d: (c, n, d[:-1] + bytes([d[-1] ^ 1])))
    chunk_fails_alone(engine, bad, 1, ZS_DATA_ERROR, "incorrect data check")


def test_a_stream_one_byte_short_or_long_of_its_chunk(engine):
    planes, _, _ = neighbours()
    raw = xc.chunk_raw(planes, RGBA, 0, 16, W, 16)

    def restream(t):
        z = zlib.compress(t, 6)
        assert len(z) < len(raw)
        return lambda c, n, d: (c, len(z), z)

    chunk_fails_alone(engine, edit_chunk_1(restream(xc.predict(raw)[:-1])), 1, ZS_DATA_ERROR, "incorrect length check")
    chunk_fails_alone(engine, edit_chunk_1(restream(xc.predict(raw) + b"\x80")), 1, ZS_DATA_ERROR, "incorrect length check")


def test_a_body_cut_by_the_files_end(engine):
    planes, good, want = neighbours()
    chunk_fails_alone(engine, good[:-1], 2, ZS_BUF_ERROR, "buffer error")
    # ... and one cut inside its chunk header
    last = exr_file_info(good)[2][2]
    chunk_fails_alone(engine, good[:last["off"] - 3], 2, ZS_BUF_ERROR, "buffer error")


def test_wrong_chunk_coordinates_and_sizes(engine):
    for what, edit, code, message in xc.CHUNK_CLAIMS:
        planes, _, _ = neighbours()
        sized = (lambda k, c, n, d: (c, 16 * W * 8 + 1, d + b"\0" * (16 * W * 8)) if k == 1 else (c, n, d)) if what == "size above U" else edit
        chunk_fails_alone(engine, xc.build(planes, W, H, RGBA, edit=sized), 1, code, message)


def test_every_file_error_and_its_message(engine):
    _, good, want = neighbours()
    for what, legal, bad, code, message in xc.CLAIMS:
        cap = max(exr_file_info(legal)[0]["out_len"], 16)
        rc, lens, codes, status, outs = run_decode(engine, [good, bad, good], caps=[want.size, cap, want.size])
        assert rc == code and status == [0, code, 0] and codes[1] == [] and lens[1] == 0, what
        assert engine.last_error() == "file 1: " + message, what
        assert np.array_equal(outs[0], want) and np.array_equal(outs[2], want) and (outs[1] == FILL).all(), what
        rc, lens, codes, status, outs = run_decode(engine, [legal])
        assert status == [0] or codes[0] != [], what  # (a legal file that was cut fails by its chunks, not as a file)


def test_decode_with_a_short_capacity(engine):
    _, good, want = neighbours()
    rc, lens, codes, status, outs = run_decode(engine, [good, good, good], caps=[want.size, want.size - 1, want.size + 5])
    assert rc == ZS_BUF_ERROR and status == [0, ZS_BUF_ERROR, 0] and lens == [want.size] * 3 and codes[1] == [] and engine.last_error() == "file 1: buffer error"
    assert np.array_equal(outs[0], want) and np.array_equal(outs[2][:want.size], want)
    assert (outs[1] == FILL).all() and (outs[2][want.size:] == FILL).all()  # nothing decoded, nothing behind out_len


def test_one_file_cut_at_every_offset_of_its_head_and_table(engine):
    """All cuts in one call, between two whole files: below 8 bytes ZS_BUF_ERROR, inside the header and the table ZS_DATA_ERROR,
    behind the table the file is walked and its chunks fail for themselves."""
    _, good, want = neighbours()
    chunks = exr_file_info(good)[2]
    bodies = chunks[0]["off"] - 8
    cuts = [good] + [good[:n] for n in range(bodies + 1)] + [good]
    rc, lens, codes, status, outs = run_decode(engine, cuts, caps=[want.size] * len(cuts))
    assert status[0] == 0 and status[-1] == 0 and np.array_equal(outs[0], want) and np.array_equal(outs[-1], want)
    for n in range(bodies + 1):
        s, c, o = status[1 + n], codes[1 + n], outs[1 + n]
        if n < 8:
            assert s == ZS_BUF_ERROR and c == [], n
        elif n < bodies:
            assert s == ZS_DATA_ERROR and c == [], n
        else:
            assert s == ZS_BUF_ERROR and c == [ZS_BUF_ERROR] * 3, n
        assert (o == FILL).all(), n
    assert rc == ZS_BUF_ERROR and engine.last_error() == "file 1: buffer error"


# ------------------------------------------------------------------ encode
def encode_shapes():
    """(planes, put fields)"""
    out = []
    for width, height, channels, kw in ((37, 53, MIXED, {}), (37, 53, RGBA, dict(compression=2)), (37, 9, MIXED, dict(compression=0)), (1, 1, RGBA, {}),
                                        (1, 40, [("Y", xc.HALF)], {}), (21, 16, RGBA, dict(x_min=-100, y_min=-7)), (21, 17, RGBA, {}),
                                        (1100, 20, RGBA, {}), (30, 20, RGBA + [("Z", xc.FLOAT)], dict(extra=xc.attr("owner", "string", b"nobody")))):
        out.append((xc.pixels(width, height, channels, seed=100 + len(out)), dict(width=width, height=height, channels=channels, **kw)))
    return out


def run_encode(engine, shapes, caps=None, level=6):
    packed = [xc.pack_planes(p, put["width"], put["height"], put["channels"], fill=FILL) for p, put in shapes]
    src = Arena([a.size for a in packed])
    for k, a in enumerate(packed):
        src.fill(k, a.tobytes())
    images = [dict(put, planes=src.ptr(k)) for k, (_, put) in enumerate(shapes)]
    bounds = [exr_bound(im) for im in images]
    caps = bounds if caps is None else caps
    out = Arena(caps)
    rc, lens, status = exr_encode(engine, images, [out.ptr(k) for k in range(len(shapes))], list(caps), level=level)
    written = [n if s == 0 else 0 for n, s in zip(lens, status)]
    files = out.results(written)
    src.results()
    assert all(n <= b for n, b in zip(lens, bounds)), "exr_bound exceeded"
    return rc, lens, status, [f[:n].tobytes() if s == 0 else b"" for f, n, s in zip(files, lens, status)]


def device_deflate(engine, buffers, level):
    """zs_deflate_batch_device on these bytes"""
    src, dst = Arena([len(b) for b in buffers]), Arena([deflate_bound(len(b)) for b in buffers])
    for k, b in enumerate(buffers):
        src.fill(k, b)
    n = len(buffers)
    lens = engine.deflate_batch_device([src.ptr(k) for k in range(n)], [len(b) for b in buffers], [dst.ptr(k) for k in range(n)], list(dst.sizes), level=level)
    return [g[:m].tobytes() for g, m in zip(dst.results(), lens)]


ATTRS = ["channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio", "screenWindowCenter", "screenWindowWidth"]


@pytest.mark.parametrize("level", [1, 6, 9])
def test_encode_and_read_it_back(engine, level):
    """One call; every file read by the model and by the decode call, its table and chunk headers field by field, every
    deflated chunk what the deflate call writes for the model's predicted bytes."""
    shapes = encode_shapes()
    rc, lens, status, files = run_encode(engine, shapes, level=level)
    assert rc == 0 and status == [0] * len(shapes), engine.last_error()
    predicted = []
    for k, ((planes, put), f) in enumerate(zip(shapes, files)):
        width, height, channels, comp = put["width"], put["height"], put["channels"], put.get("compression", 3)
        info, got_channels, got, chunks = xc.read(f)
        assert f[:8] == xc.MAGIC + b"\2\0\0\0" and got_channels == channels and np.array_equal(got, xc.pack_planes(planes, width, height, channels)), (k, put)
        x0, y0 = put.get("x_min", 0), put.get("y_min", 0)
        assert info["data_window"] == info["display_window"] == (x0, y0, x0 + width - 1, y0 + height - 1) and (info["compression"], info["line_order"]) == (comp, 0)
        assert list(info["attrs"]) == ATTRS + (["owner"] if "extra" in put else [])
        a = info["attrs"]
        assert a["pixelAspectRatio"] == ("float", struct.pack("<f", 1.0)) and a["screenWindowCenter"] == ("v2f", struct.pack("<2f", 0, 0)) and a["screenWindowWidth"] == ("float", struct.pack("<f", 1.0))
        if "extra" in put:
            assert a["owner"] == ("string", b"nobody")
        # the table and the chunk headers: ascending, back to back from the table's end to the file's
        lines = 16 if comp == 3 else 1
        at = chunks[0]["at"]
        table_at = at - 8 * len(chunks)
        assert f[table_at - 1] == 0 and len(chunks) == -(-height // lines)
        for j, c in enumerate(chunks):
            assert struct.unpack_from("<Q", f, table_at + 8 * j)[0] == c["at"] == at
            assert struct.unpack_from("<ii", f, at) == (y0 + j * lines, c["size"]) and (c["y"], c["h"]) == (j * lines, min(lines, height - j * lines))
            at += 8 + c["size"]
            raw = xc.chunk_raw(planes, channels, 0, c["y"], width, c["h"])
            body = f[c["off"]:c["off"] + c["size"]]
            if comp == 0:
                assert body == raw
            elif c["size"] < c["raw_len"]:
                predicted.append((xc.predict(raw), body))
            else:
                assert body == raw
        assert at == len(f)
    assert len(predicted) >= 10
    for j, (z, (p, body)) in enumerate(zip(device_deflate(engine, [p for p, _ in predicted], level), predicted)):
        assert z == body and zlib.decompress(body) == p, j
    rc, lens, codes, status, outs = run_decode(engine, files)
    assert rc == 0 and status == [0] * len(files)
    for (planes, put), got in zip(shapes, outs):
        assert np.array_equal(got, expect(planes, put["width"], put["height"], put["channels"])), put


def test_a_noise_image_is_stored_raw(engine):
    planes = xc.pixels(40, 40, RGBA, seed=120, noise=True)
    smooth = xc.pixels(40, 40, RGBA, seed=121)
    for name, _ in RGBA:
        planes[name][32:] = smooth[name][32:]  # the last chunk deflates, the two in front of it do not
    rc, lens, status, files = run_encode(engine, [(planes, dict(width=40, height=40, channels=RGBA))])
    assert rc == 0 and status == [0]
    info, channels, chunks = exr_file_info(files[0])
    assert [c["data_len"] == c["raw_len"] for c in chunks] == [True, True, False] and chunks[0]["raw_len"] == 16 * 40 * 8
    for c in chunks[:2]:
        assert files[0][c["off"]:c["off"] + c["data_len"]] == xc.chunk_raw(planes, RGBA, 0, c["y"], 40, c["h"])
    assert np.array_equal(xc.read(files[0])[2], xc.pack_planes(planes, 40, 40, RGBA))
    rc, _, _, status, outs = run_decode(engine, files)
    assert rc == 0 and np.array_equal(outs[0], expect(planes, 40, 40, RGBA))


def test_encode_with_a_short_capacity(engine):
    shapes = encode_shapes()[:3]
    _, lens, _, files = run_encode(engine, shapes)
    rc, lens2, status, files2 = run_encode(engine, shapes, caps=[lens[0], lens[1] - 1, lens[2] + 7])
    assert rc == ZS_BUF_ERROR and status == [0, ZS_BUF_ERROR, 0] and lens2 == lens and engine.last_error() == "buffer error"
    assert files2[0] == files[0] and files2[2] == files[2]


def test_encode_refuses_before_device_work(engine):
    a = Arena([1 << 12, 1 << 12])
    for channels in ([("R", xc.HALF), ("G", xc.HALF)], [("G", xc.HALF), ("G", xc.HALF)], [("n" * 32, xc.HALF)], []):
        with pytest.raises(ValueError):
            exr_encode(engine, [dict(planes=a.ptr(0), width=4, height=4, channels=channels)], [a.ptr(1)], [1 << 12])
    with pytest.raises(ValueError):
        exr_encode(engine, [dict(planes=a.ptr(0), width=4, height=4, channels=RGBA, compression=4)], [a.ptr(1)], [1 << 12])
    a.results([0, 0])
