"""TIFF files on the device, both directions (include/zsgpu.h zs_tiff_*).  Ground truth is always the numpy array a file was
built from (tests/tiff_cases.py builds and reads files in pure Python; tests/golden/tiff holds files libtiff wrote); Pillow is a
second witness for the shapes it handles.  The predictor kernels are held against numpy alone first: every sample size, 1 .. 8
samples per pixel, both byte orders, rows around one wave pass (1024 bytes), all-ones differences, clipped tiles, outputs at odd
addresses between guard bytes.  Images are at most ~300 pixels a side."""
import io
import os
import zlib

import numpy as np
import pytest

import tiff_cases as tc
from zlibstream_amd import tiff_bound, tiff_decode_files, tiff_encode, tiff_file_info, tiff_predict, tiff_unpredict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff")
GUARD, FILL = 64, 0xEE
ZS_DATA_ERROR, ZS_BUF_ERROR = -3, -5


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
def kernel_cases():
    """(rows of the image part, width, spp, bits, fmt, predictor, order, chunk width, chunk height): the chunk is cut from the
    image with its surplus repeated, as a writer pads a tile."""
    out = []
    for width in (1, 2, 63, 64, 65):
        for spp in range(1, 9):
            for bits in (8, 16, 32):
                for order in "<>":
                    out.append((tc.pixels(width, 3, spp, bits, seed=20), width, spp, bits, 1, 2, order, width, 3))
    # rows of 1023, 1024, 1025 and 2049 bytes: one wave pass, and the carry into the next
    for nbytes in (1023, 1024, 1025, 2049):
        out.append((tc.pixels(nbytes, 2, 1, 8, seed=21), nbytes, 1, 8, 1, 2, "<", nbytes, 2))
    for width, spp, bits in ((341, 3, 8), (683, 3, 8), (205, 5, 8), (512, 1, 16), (513, 1, 16), (171, 3, 16), (256, 1, 32), (257, 1, 32), (37, 7, 32), (300, 6, 16)):
        for order in "<>":
            out.append((tc.pixels(width, 2, spp, bits, seed=22), width, spp, bits, 1, 2, order, width, 2))
    # differences of all ones: every sum carries through all bytes of a sample
    for spp, bits in ((1, 16), (3, 16), (1, 32), (4, 32)):
        for order in "<>":
            out.append((tc.all_ff_differences(600, 2, spp, bits), 600, spp, bits, 1, 2, order, 600, 2))
    # the floating-point predictor
    for spp in (1, 3, 4):
        for width in (1, 2, 63, 65, 300):
            for order in "<>":
                out.append((tc.pixels(width, 3, spp, 32, seed=23, fmt=3), width, spp, 32, 3, 3, order, width, 3))
    # tiles that hang over the image: 37 x 21 pixels in a chunk of 48 x 32
    for spp, bits, fmt, predictor in ((3, 8, 1, 2), (4, 16, 1, 2), (1, 32, 3, 3), (3, 32, 3, 3), (2, 16, 1, 1), (1, 8, 1, 1)):
        out.append((tc.pixels(37, 21, spp, bits, seed=24, fmt=fmt), 37, spp, bits, fmt, predictor, ">" if predictor == 1 else "<", 48, 32))
    # predictor 1: a copy, swapped for big-endian samples; below 8 bits the bytes as they are
    for bits in (16, 32):
        out.append((tc.pixels(100, 3, 3, bits, seed=25), 100, 3, bits, 1, 1, ">", 100, 3))
    out.append((tc.pixels(96, 5, 1, 1, seed=26), 96, 1, 1, 1, 1, "<", 96, 5))
    out.append((tc.pixels(33, 5, 3, 4, seed=27), 33, 3, 4, 1, 1, ">", 33, 5))
    return out


def test_undo_kernel_against_numpy(engine):
    cases = kernel_cases()
    chunks = [tc.predict(tc.cut(rows, w, spp, bits, 0, 0, cw, ch), spp, bits, p, order) for rows, w, spp, bits, fmt, p, order, cw, ch in cases]
    src, dst = Arena([c.size for c in chunks]), Arena([c[0].size for c in cases])
    for k, c in enumerate(chunks):
        src.fill(k, c.tobytes())
    n = len(cases)
    tiff_unpredict(engine, [src.ptr(k) for k in range(n)], [dst.ptr(k) for k in range(n)], [c[7] for c in cases], [c[8] for c in cases], [c[3] for c in cases],
                   [c[2] for c in cases], [c[5] for c in cases], out_widths=[c[1] for c in cases], out_heights=[c[0].shape[0] for c in cases],
                   big_endian=[int(c[6] == ">") for c in cases])
    for k, (got, c) in enumerate(zip(dst.results(), cases)):
        assert np.array_equal(got, c[0].reshape(-1)), "case %d: width %d spp %d bits %d predictor %d order %s chunk %d x %d" % ((k,) + c[1:4] + c[5:])


def test_forward_kernel_against_numpy_and_back(engine):
    """The forward kernel cuts, pads and predicts as numpy does; the undo kernel gives the image back."""
    cases = [c for c in kernel_cases() if c[6] == "<" or c[5] == 1 and c[3] < 8]  # (the writer is little-endian)
    want = [tc.predict(tc.cut(rows, w, spp, bits, 0, 0, cw, ch), spp, bits, p, "<") for rows, w, spp, bits, fmt, p, order, cw, ch in cases]
    img, mid, back = Arena([c[0].size for c in cases]), Arena([w.size for w in want]), Arena([c[0].size for c in cases])
    for k, c in enumerate(cases):
        img.fill(k, c[0].tobytes())
    n = len(cases)
    bits, spp, pred = [c[3] for c in cases], [c[2] for c in cases], [c[5] for c in cases]
    tiff_predict(engine, [img.ptr(k) for k in range(n)], [mid.ptr(k) for k in range(n)], [c[1] for c in cases], [c[0].shape[0] for c in cases], bits, spp, pred,
                 widths=[c[7] for c in cases], heights=[c[8] for c in cases])
    for k, (got, w) in enumerate(zip(mid.results(), want)):
        assert np.array_equal(got, w.reshape(-1)), "case %d: %s" % (k, cases[k][1:])
    tiff_unpredict(engine, [mid.ptr(k) for k in range(n)], [back.ptr(k) for k in range(n)], [c[7] for c in cases], [c[8] for c in cases], bits, spp, pred,
                   out_widths=[c[1] for c in cases], out_heights=[c[0].shape[0] for c in cases])
    for k, (got, c) in enumerate(zip(back.results(), cases)):
        assert np.array_equal(got, c[0].reshape(-1)), "case %d: %s" % (k, c[1:])


# ------------------------------------------------------------------ decode
def run_decode(engine, files, pages=None, caps=None):
    """zs_tiff_decode_files_batch with every output at an odd address between guard bytes.  caps: None for each page's out_len.
    Returns (code, out_len[], chunk codes[][], status[], the outputs)."""
    if caps is None:
        caps = [tiff_file_info(f, pages[i] if pages else 0)[0]["out_len"] for i, f in enumerate(files)]
    out = Arena(caps)
    rc, lens, codes, status = tiff_decode_files(engine, files, [out.ptr(k) for k in range(len(files))], list(caps), pages=pages)
    return rc, lens, codes, status, out.results()


def check_decoded(engine, files, rows, pages=None):
    rc, lens, codes, status, outs = run_decode(engine, files, pages)
    assert rc == 0 and status == [0] * len(files), (rc, status, engine.last_error())
    for k, (f, r, n, c, o) in enumerate(zip(files, rows, lens, codes, outs)):
        assert n == r.size == o.size and c == [0] * len(c) and len(c) >= 1, k
        assert np.array_equal(o, r.reshape(-1)), "file %d differs, first at byte %d" % (k, int(np.flatnonzero(o != r.reshape(-1))[0]))


def golden_files():
    return [open(os.path.join(GOLDEN, g[0] + ".tif"), "rb").read() for g in tc.GOLDEN], [tc.golden_rows(g[0]) for g in tc.GOLDEN]


_CACHE = {}


def built_files():
    """(name, file, rows, page): every layout the reader knows, made once."""
    if "built" not in _CACHE:
        _CACHE["built"] = _built_files()
    return _CACHE["built"]


def _built_files():
    out = []
    rgb, g16, rgba16, u32, f1, f3 = (tc.pixels(37, 53, 3, 8, seed=30), tc.pixels(37, 53, 1, 16, seed=31), tc.pixels(37, 53, 4, 16, seed=32),
                                     tc.pixels(37, 53, 2, 32, seed=33), tc.pixels(37, 53, 1, 32, seed=34, fmt=3), tc.pixels(37, 53, 3, 32, seed=35, fmt=3))
    for order in "<>":
        o = "II" if order == "<" else "MM"
        out.append((o + " rgb p2 strips, short last", tc.simple(rgb, 37, 3, 8, order=order, predictor=2, rows_per_strip=10), rgb, 0))
        out.append((o + " rgb p2 strips, padded last", tc.simple(rgb, 37, 3, 8, order=order, predictor=2, rows_per_strip=10, pad_last_strip=True), rgb, 0))
        out.append((o + " rgb p1 strips, padded last", tc.simple(rgb, 37, 3, 8, order=order, rows_per_strip=10, pad_last_strip=True), rgb, 0))
        out.append((o + " gray16 p1 strips", tc.simple(g16, 37, 1, 16, order=order, rows_per_strip=7), g16, 0))
        out.append((o + " gray16 p2 tiles", tc.simple(g16, 37, 1, 16, order=order, predictor=2, tile=(16, 16)), g16, 0))
        out.append((o + " rgba16 p2 tiles 16x32", tc.simple(rgba16, 37, 4, 16, order=order, predictor=2, tile=(16, 32), extra=[2]), rgba16, 0))
        out.append((o + " u32x2 p2 strips", tc.simple(u32, 37, 2, 32, order=order, predictor=2, rows_per_strip=20), u32, 0))
        out.append((o + " float p3 strips", tc.simple(f1, 37, 1, 32, order=order, fmt=3, predictor=3, rows_per_strip=9), f1, 0))
        out.append((o + " float x3 p3 tiles", tc.simple(f3, 37, 3, 32, order=order, fmt=3, predictor=3, tile=(16, 16)), f3, 0))
        out.append((o + " float p1 tiles", tc.simple(f1, 37, 1, 32, order=order, fmt=3, tile=(32, 32)), f1, 0))
        out.append((o + " bigtiff rgb tiles, odd offsets", tc.simple(rgb, 37, 3, 8, order=order, big=True, predictor=2, tile=(16, 16), odd_offsets=True), rgb, 0))
        out.append((o + " uncompressed gray16 p2 tiles, odd offsets", tc.simple(g16, 37, 1, 16, order=order, predictor=2, compression=1, tile=(16, 16), odd_offsets=True), g16, 0))
        out.append((o + " uncompressed rgb strips", tc.simple(rgb, 37, 3, 8, order=order, compression=1, rows_per_strip=10), rgb, 0))
    one_tile, one_px = tc.pixels(16, 16, 3, 8, seed=36), tc.pixels(1, 1, 3, 16, seed=37)
    out.append(("one tile", tc.simple(one_tile, 16, 3, 8, predictor=2, tile=(16, 16)), one_tile, 0))
    out.append(("one pixel", tc.simple(one_px, 1, 3, 16, predictor=2, order=">"), one_px, 0))
    out.append(("one pixel in a tile", tc.simple(one_px, 1, 3, 16, predictor=2, tile=(16, 16)), one_px, 0))
    out.append(("compression 32946", tc.simple(rgb, 37, 3, 8, predictor=2, compression=32946, rows_per_strip=10), rgb, 0))
    for bits in (1, 2, 4):
        sub = tc.pixels(45, 19, 1, bits, seed=38)
        out.append(("%d-bit strips" % bits, tc.simple(sub, 45, 1, bits, rows_per_strip=4, odd_offsets=True), sub, 0))
        out.append(("%d-bit tiles" % bits, tc.simple(sub, 45, 1, bits, tile=(32, 16)), sub, 0))
    big = tc.pixels(301, 290, 3, 8, seed=39)  # strips of 30 KB, compressed above the one-wave decoder's 1 KiB
    out.append(("rgb 301 x 290 p2", tc.simple(big, 301, 3, 8, predictor=2, rows_per_strip=33), big, 0))
    out.append(("rgb 301 x 290 p1 tiles 128", tc.simple(big, 301, 3, 8, tile=(128, 128)), big, 0))
    two = tc.build([tc.page(rgb, 37, 3, 8, predictor=2, rows_per_strip=10), tc.page(g16, 37, 1, 16, predictor=2, tile=(16, 16))])
    out.append(("page 1 of two", two, g16, 1))
    out.append(("page 0 of two", two, rgb, 0))
    return out


def test_decode_the_golden_files(engine):
    """What libtiff wrote, one call; and each file alone is what Pillow reads from it."""
    files, rows = golden_files()
    check_decoded(engine, files, rows)
    Image = pytest.importorskip("PIL.Image")
    for g, f, r in zip(tc.GOLDEN, files, rows):
        if g[1] != "1":
            assert np.asarray(Image.open(io.BytesIO(f))).tobytes() == r.tobytes(), g[0]


@pytest.mark.parametrize("k", range(0, 41, 7))
def test_decode_built_files_one_at_a_time(engine, k):
    cases = built_files()[k:k + 7]
    for name, f, r, page in cases:
        rc, lens, codes, status, outs = run_decode(engine, [f], [page])
        assert rc == 0 and np.array_equal(outs[0], r.reshape(-1)), (name, rc, engine.last_error())


def test_decode_everything_in_one_call(engine):
    cases = built_files()
    assert len(cases) <= 41
    gf, gr = golden_files()
    check_decoded(engine, [c[1] for c in cases] + gf, [c[2] for c in cases] + gr, pages=[c[3] for c in cases] + [0] * len(gf))


def corrupt(kind):
    """A 48 x 48 rgb file of nine 16 x 16 tiles (or, for the strip kinds, of six strips) whose chunk 4 (3) is damaged."""
    rows = tc.pixels(48, 48, 3, 8, seed=40)

    def edit(k, body, at=4):
        if k != at:
            return body
        if kind == "adler":
            return body[:-1] + bytes([body[-1] ^ 1])
        if kind == "flipped bit":
            raw = zlib.decompress(body)
            return zlib.compress(raw[:100] + bytes([raw[100] ^ 8]) + raw[101:])[:-4] + body[-4:]
        if kind == "truncated":
            return body[:len(body) // 2]
        if kind == "tile decoding short":
            return zlib.compress(zlib.decompress(body)[:-1])
        if kind == "tile decoding long":
            return zlib.compress(zlib.decompress(body) + b"\0")
        if kind == "header":
            return b"\x78\x9d" + body[2:]
        return body

    if kind == "strip decoding short":
        return rows, tc.simple(rows, 48, 3, 8, predictor=2, rows_per_strip=8, chunk_edit=lambda k, b: zlib.compress(zlib.decompress(b)[:-1]) if k == 3 else b), 3
    if kind == "own strip decoding long":
        return rows, tc.simple(rows, 48, 3, 8, rows_per_strip=8, chunk_edit=lambda k, b: zlib.compress(zlib.decompress(b) + b"\0") if k == 3 else b), 3
    if kind == "uncompressed short":
        f = tc.simple(rows, 48, 3, 8, compression=1, tile=(16, 16))
        return rows, _with_count(bytearray(f), tc.read_ifds(f)[0][0], 4, 767), 4
    return rows, tc.simple(rows, 48, 3, 8, predictor=2, tile=(16, 16), chunk_edit=edit), 4


def _with_count(f, tags, k, value):
    """The file with chunk k's byte count replaced (classic little-endian, counts out of line)."""
    counts = b"".join(int(v).to_bytes(4, "little") for v in tags[325])
    at = bytes(f).index(counts)
    f[at + 4 * k:at + 4 * k + 4] = int(value).to_bytes(4, "little")
    return bytes(f)


BAD = {"adler": (ZS_DATA_ERROR, "incorrect data check"), "flipped bit": (ZS_DATA_ERROR, "incorrect data check"), "truncated": (ZS_BUF_ERROR, "buffer error"),
       "tile decoding short": (ZS_DATA_ERROR, "incorrect length check"), "tile decoding long": (ZS_DATA_ERROR, "incorrect length check"),
       "header": (ZS_DATA_ERROR, "incorrect header check"), "strip decoding short": (ZS_DATA_ERROR, "incorrect length check"),
       "own strip decoding long": (ZS_DATA_ERROR, "incorrect length check"), "uncompressed short": (ZS_DATA_ERROR, "incorrect length check")}


def test_a_corrupt_chunk_fails_for_itself_only(engine):
    """Every kind of damage in one call, each between whole files: the damaged chunk's code and reason, every other chunk of
    its file byte-exact, the neighbours whole."""
    good_rows = tc.pixels(37, 53, 3, 8, seed=41)
    good = tc.simple(good_rows, 37, 3, 8, predictor=2, tile=(16, 16))
    kinds = list(BAD)
    made = [corrupt(k) for k in kinds]
    files = [good] + [x for _, f, _ in made for x in (f, good)]
    rc, lens, codes, status, outs = run_decode(engine, files)
    assert rc == BAD[kinds[0]][0] and engine.last_error() == "file 1: chunk %d: %s" % (made[0][2], BAD[kinds[0]][1]), (rc, engine.last_error())
    for k in range(0, len(files), 2):
        assert status[k] == 0 and codes[k] == [0] * 12 and np.array_equal(outs[k], good_rows.reshape(-1)), k
    for j, (kind, (rows, f, bad)) in enumerate(zip(kinds, made)):
        k = 2 * j + 1
        want = [0] * len(codes[k])
        want[bad] = BAD[kind][0]
        assert status[k] == BAD[kind][0] and codes[k] == want, (kind, status[k], codes[k])
        info, chunks = tiff_file_info(f)
        got = outs[k].reshape(48, -1)
        for i, c in enumerate(chunks):
            if i != bad:
                part = (slice(c["y"], c["y"] + c["h"]), slice(c["x"] * 3, (c["x"] + c["w"]) * 3))
                assert np.array_equal(got[part], rows[part]), (kind, i)
        # each alone: the same code, and the reason
        rc1, _, codes1, status1, _ = run_decode(engine, [f])
        assert rc1 == BAD[kind][0] and codes1[0] == want and engine.last_error() == "file 0: chunk %d: %s" % (bad, BAD[kind][1]), (kind, engine.last_error())


def test_every_cut_of_one_file_in_one_call(engine):
    """Every prefix of a small file: no fault, the class the file's layout gives, and the chunks that are whole decode."""
    rows = tc.pixels(20, 12, 1, 8, seed=42)
    f = tc.simple(rows, 20, 1, 8, predictor=2, rows_per_strip=4)
    info, chunks = tiff_file_info(f)
    head = min(c["off"] for c in chunks)  # header, IFD and its values lie in front of the chunks
    cuts = [f[:n] for n in range(len(f))]
    rc, lens, codes, status, outs = run_decode(engine, cuts, caps=[rows.size] * len(cuts))
    for n, (s, c, o) in enumerate(zip(status, codes, outs)):
        if n < 8:
            assert s == ZS_BUF_ERROR and c == [], n
        elif n < head:
            assert s == ZS_DATA_ERROR and c == [], n
        else:
            whole = [ch["off"] + ch["comp_len"] <= n for ch in chunks]
            assert c == [0 if w else ZS_BUF_ERROR for w in whole] and s == ZS_BUF_ERROR, (n, c, s)
            got = o.reshape(12, -1)
            for ch, w in zip(chunks, whole):
                if w:
                    assert np.array_equal(got[ch["y"]:ch["y"] + ch["h"]], rows[ch["y"]:ch["y"] + ch["h"]]), n
    assert rc == ZS_BUF_ERROR and engine.last_error().startswith("file 0: ")


def test_decode_with_a_short_capacity(engine):
    rows = tc.pixels(37, 53, 3, 8, seed=43)
    f = tc.simple(rows, 37, 3, 8, predictor=2, rows_per_strip=10)
    rc, lens, codes, status, outs = run_decode(engine, [f, f, f], caps=[rows.size, rows.size - 1, rows.size + 5])
    assert rc == ZS_BUF_ERROR and status == [0, ZS_BUF_ERROR, 0] and lens == [rows.size] * 3 and codes[1] == [] and engine.last_error() == "file 1: buffer error"
    assert np.array_equal(outs[0], rows.reshape(-1)) and np.array_equal(outs[2][:rows.size], rows.reshape(-1))
    assert (outs[1] == FILL).all() and (outs[2][rows.size:] == FILL).all()  # nothing decoded, nothing behind out_len


# ------------------------------------------------------------------ encode
def encode_shapes():
    """(rows, put fields): every shape the writer knows."""
    out = []
    for spp, bits, fmt in ((1, 8, 1), (2, 8, 1), (3, 8, 1), (4, 8, 1), (1, 16, 1), (3, 16, 1), (4, 16, 1), (1, 32, 1), (2, 32, 1), (1, 32, 3), (3, 32, 3), (5, 8, 1), (8, 16, 1)):
        rows = tc.pixels(37, 53, spp, bits, seed=50, fmt=fmt)
        base = dict(width=37, height=53, spp=spp, bits=bits, sample_format=fmt, photometric=2 if spp >= 3 else 1,
                    extra_samples=spp - 3 if spp > 3 else (1 if spp == 2 else 0), extra_kind=2 if spp in (2, 4) else 0)
        for predictor in (1, 2) + ((3,) if fmt == 3 else ()):
            out.append((rows, dict(base, predictor=predictor, rows_per_strip=10)))
            out.append((rows, dict(base, predictor=predictor, tile_width=16, tile_height=32)))
    for bits in (1, 4):
        rows = tc.pixels(45, 19, 1, bits, seed=51)
        out.append((rows, dict(width=45, height=19, bits=bits, rows_per_strip=4)))
        out.append((rows, dict(width=45, height=19, bits=bits, tile_width=32, tile_height=16)))
    big = tc.pixels(301, 290, 3, 8, seed=52)
    out.append((big, dict(width=301, height=290, spp=3, photometric=2, predictor=2)))  # rows_per_strip 0: the default, one strip here
    out.append((big, dict(width=301, height=290, spp=3, photometric=2, predictor=2, tile_width=128, tile_height=128)))
    one = tc.pixels(1, 1, 3, 16, seed=53)
    out.append((one, dict(width=1, height=1, spp=3, bits=16, photometric=2, predictor=2)))
    return out


def run_encode(engine, shapes, caps=None, level=6):
    src = Arena([r.size for r, _ in shapes])
    for k, (r, _) in enumerate(shapes):
        src.fill(k, r.tobytes())
    images = [dict(put, pixels=src.ptr(k)) for k, (_, put) in enumerate(shapes)]
    bounds = [tiff_bound(im) for im in images]
    caps = bounds if caps is None else caps
    out = Arena(caps)
    rc, lens, status = tiff_encode(engine, images, [out.ptr(k) for k in range(len(shapes))], list(caps), level=level)
    written = [n if s == 0 else 0 for n, s in zip(lens, status)]
    files = out.results(written)
    assert all(n <= b for n, b in zip(lens, bounds)), "tiff_bound exceeded"
    return rc, lens, status, [f[:n].tobytes() if s == 0 else b"" for f, n, s in zip(files, lens, status)]


def test_encode_every_shape_and_read_it_back(engine):
    """One call; every file read by the pure-Python reader, by Pillow where it handles the shape, and by the decode call;
    every chunk's stream is what the deflate call writes for numpy's predicted bytes."""
    shapes = encode_shapes()
    rc, lens, status, files = run_encode(engine, shapes)
    assert rc == 0 and status == [0] * len(shapes), engine.last_error()
    predicted = []
    for k, ((rows, put), f) in enumerate(zip(shapes, files)):
        tags, got = tc.read(f)
        assert np.array_equal(got, rows), (k, put)
        info, chunks = tiff_file_info(f)
        assert f[:4] == b"II*\0" and sorted(tags) == list(tags) and all(c["off"] % 2 == 0 and c["status"] == 0 for c in chunks), (k, put)
        assert (info["compression"], info["predictor"], info["planar"], info["n_pages"]) == (8, put.get("predictor", 1), 1, 1)
        assert (info["sample_format"], info["photometric"], info["extra_samples"]) == (put.get("sample_format", 1), put.get("photometric", 1), put.get("extra_samples", 0))
        assert info["tiled"] == int("tile_width" in put) and chunks[-1]["off"] + chunks[-1]["comp_len"] + (chunks[-1]["comp_len"] & 1) == len(f)
        spp, bits = put.get("spp", 1), put.get("bits", 8)
        for c in chunks:
            ch = info["chunk_h"] if info["tiled"] else c["h"]
            padded = tc.cut(rows, put["width"], spp, bits, c["x"], c["y"], info["chunk_w"], ch)
            if bits < 8 and c["w"] < info["chunk_w"]:
                n_in = tc.row_bytes(c["w"], spp, bits)
                padded[:, n_in:] = padded[:, n_in - 1:n_in]
            predicted.append((tc.predict(padded, spp, bits, info["predictor"]).tobytes(), f[c["off"]:c["off"] + c["comp_len"]]))
    streams = engine.deflate_batch([p for p, _ in predicted], level=6)
    for k, (z, (p, body)) in enumerate(zip(streams, predicted)):
        assert z == body and zlib.decompress(body) == p, k
    Image = pytest.importorskip("PIL.Image")
    seen = 0
    for (rows, put), f in zip(shapes, files):
        spp, bits, fmt = put.get("spp", 1), put.get("bits", 8), put.get("sample_format", 1)
        if (bits == 8 and spp <= 4) or (bits == 16 and spp == 1) or (fmt == 3 and spp == 1):
            assert np.asarray(Image.open(io.BytesIO(f))).tobytes() == rows.tobytes(), put
            seen += 1
    assert seen >= 14


def test_decode_of_encode_is_the_identity_for_a_mixed_batch(engine):
    shapes = encode_shapes()[::3]
    rc, lens, status, files = run_encode(engine, shapes, level=1)
    assert rc == 0
    check_decoded(engine, files, [r for r, _ in shapes])


def test_encode_with_a_short_capacity(engine):
    shapes = encode_shapes()[:3]
    _, lens, _, files = run_encode(engine, shapes)
    rc, lens2, status, files2 = run_encode(engine, shapes, caps=[lens[0], lens[1] - 1, lens[2] + 7])
    assert rc == ZS_BUF_ERROR and status == [0, ZS_BUF_ERROR, 0] and lens2 == lens and engine.last_error() == "buffer error"
    assert files2[0] == files[0] and files2[2] == files[2] and files2[1] == b""  # (run_encode checks that nothing was written for it)
