"""The batched PNG encoder on the device: zs_deflate_writes_batch_device (n streams, each in its own NoFlush Writes),
zs_png_filter_batch_device (one launch over the rows of n images) and zs_png_idat_batch_device (pixels in HBM -> IDAT payloads in
HBM).  Expected bytes come from the oracle's WriteCore loop (oracle.compress(data, level, strategy, chunks=sizes)) and from a
numpy restatement of PNG specification 9.2, never from the library; every comparison is exact."""
import ctypes
import zlib

import numpy as np
import pytest

import oracle_binding
from zlibstream_amd import datagen, deflate_bound

pytestmark = pytest.mark.gpu

ZS_OK, ZS_BUF_ERROR = 0, -5


# ---------------------------------------------------------------- helpers
def _ends_of(n, spec, rng):
    """Cumulative Write ends of an n-byte stream: spec an int (that size every Write), ("r", lo, hi) random odd sizes, or a
    list of sizes used in turn."""
    ends, o = [], 0
    while o < n:
        if isinstance(spec, int):
            w = spec
        elif spec[0] == "r":
            w = int(rng.integers(spec[1], spec[2] + 1)) | 1
        else:
            w = spec[len(ends) % len(spec)]
        o = min(n, o + max(1, w))
        ends.append(o)
    return ends


def _sizes(ends):
    """The non-empty Writes of a list of cumulative ends: what reaches Deflate, and what the oracle is given."""
    out, prev = [], 0
    for e in ends:
        if e > prev:
            out.append(e - prev)
        prev = e
    return out


def _mixed_streams():
    """(name, data, write ends or None) -- about 19 MiB: the kinds of schedule a caller brings, and the three that end on the
    one-wave literal engine today."""
    rng = np.random.default_rng(2024)
    text = datagen.english(8 << 20, 31)
    rows = datagen.sparse(512, 512)
    odd = datagen.english(2 << 20, 77)
    gaps = datagen.english(1 << 20, 5) + datagen.sparse(256, 512)
    wide = oracle_binding.corpus("ptt5") + datagen.english(2500000, 9)
    scan = datagen.sparse(4096, 12)[:16385 * 12]
    near = datagen.english(200000, 13)
    gap_ends = []
    for k, e in enumerate(_ends_of(len(gaps), [30000, 1, 4097, 65536], rng)):
        gap_ends += [e] * (1 + k % 3)  # repeated ends: empty Writes
    return [
        ("english, 81 920-byte Writes", text, _ends_of(len(text), 81920, rng)),
        ("sparse rows, a Write per row", rows, _ends_of(len(rows), 2048, rng)),
        ("no list", datagen.english(3 << 20, 3), None),
        ("random odd sizes", odd, _ends_of(len(odd), ("r", 1001, 90001), rng)),
        ("repeated ends", gaps, [0, 0] + gap_ends + [len(gaps)]),  # (also an empty first and last Write)
        ("3 bytes a Write", datagen.english(12000, 11), _ends_of(12000, 3, rng)),
        ("under 262 bytes", text[:200], [50, 50, 200]),
        ("across window ends, 100 000-byte Writes", wide, _ends_of(len(wide), 100000, rng)),
        ("16 385-byte scanlines", scan, _ends_of(len(scan), 16385, rng)),
        ("an end 100 bytes below a window end", near, [65436, 98254, len(near)]),
        ("one end only", text[:70000], [70000]),
    ]


class _Dev:
    """Streams and their output buffers on the device."""

    def __init__(self, datas, caps=None):
        import torch
        self.n = len(datas)
        self.lens = [len(d) for d in datas]
        self.d_in = [torch.frombuffer(bytearray(d) + bytearray(64), dtype=torch.uint8).cuda() for d in datas]
        self.caps = list(caps) if caps is not None else [deflate_bound(n) + 4096 for n in self.lens]
        self.d_out = [torch.full((c + 64,), 0xEE, dtype=torch.uint8, device="cuda") for c in self.caps]
        torch.cuda.synchronize()  # torch works on its own stream; the engine's stream does not wait for that one

    def in_ptrs(self):
        return [t.data_ptr() for t in self.d_in]

    def out_ptrs(self):
        return [t.data_ptr() for t in self.d_out]

    def result(self, i, n):
        return self.d_out[i][:n].cpu().numpy().tobytes()


def _alone(engine, data, ends, level, strategy):
    """One stream through zs_deflate_writes_device (no list: zs_deflate_batch_device with one stream)."""
    d = _Dev([data])
    if ends is None:
        n = engine.deflate_batch_device(d.in_ptrs(), d.lens, d.out_ptrs(), d.caps, level=level, strategy=strategy)[0]
    else:
        n = engine.deflate_writes_device(d.in_ptrs()[0], len(data), ends, d.out_ptrs()[0], d.caps[0], level=level, strategy=strategy)
    return d.result(0, n)


# ---------------------------------------------------------------- 1. the deflate of a batch of Write lists
CONFIGS = [(0, 0), (1, 0), (3, 0), (4, 0), (6, 0), (9, 0), (6, 1), (6, 2), (6, 3), (6, 4)]


@pytest.mark.parametrize("level,strategy", CONFIGS)
def test_mixed_batch_is_the_oracles_bytes_and_every_stream_takes_the_path_it_takes_alone(engine, oracle, level, strategy):
    """One call for eleven streams of every kind of schedule: each stream is the oracle's WriteCore loop on its own Writes, byte
    for byte.  Then the same streams one by one through zs_deflate_writes_device: the same bytes again, and the literal
    engine's counter grows over the batch call by exactly the sum of what it grows for the streams alone -- no stream is moved
    to the literal engine, or off it, because it has neighbours."""
    streams = _mixed_streams()
    assert 18 << 20 < sum(len(d) for _, d, _ in streams) < 22 << 20
    d = _Dev([data for _, data, _ in streams])
    before = engine.counter("lit_engine_bytes")
    lens = engine.deflate_writes_batch_device(d.in_ptrs(), d.lens, [e for _, _, e in streams], d.out_ptrs(), d.caps, level=level, strategy=strategy)
    lit_batch = engine.counter("lit_engine_bytes") - before
    got = [d.result(i, lens[i]) for i in range(d.n)]
    for (name, data, ends), z in zip(streams, got):
        want = oracle.compress(data, level, strategy, chunks=_sizes(ends) if ends is not None else None)
        assert z == want, "level %d strategy %d, %s: %d bytes against the oracle's %d" % (level, strategy, name, len(z), len(want))
    lit_alone = 0
    for (name, data, ends), z in zip(streams, got):
        before = engine.counter("lit_engine_bytes")
        z1 = _alone(engine, data, ends, level, strategy)
        grew = engine.counter("lit_engine_bytes") - before
        print("level %d strategy %d, %-42s %8d bytes, literal engine alone: %d" % (level, strategy, name, len(data), grew))
        lit_alone += grew
        assert z1 == z, "level %d strategy %d, %s: the batch's bytes differ from the stream's own call" % (level, strategy, name)
    print("level %d strategy %d: literal engine bytes: batch %d, one by one %d" % (level, strategy, lit_batch, lit_alone))
    assert lit_batch == lit_alone, "level %d strategy %d: %d bytes on the literal engine in the batch, %d one by one" % (level, strategy, lit_batch, lit_alone)
    if level >= 1 and strategy != 3:
        assert lit_batch >= 12000 - 261, "the stream written 3 bytes at a time is the literal engine's"


def test_no_lists_at_all_is_the_plain_batch_and_single_writes_keep_the_speculative_walk(engine, oracle):
    """write_ends == NULL is zs_deflate_batch_device on the same buffers; and in a batch that has lists, the streams without
    one (1 MiB of text each at level 6) still take the speculative chunk walk, as `spec_streams` shows."""
    texts = [datagen.english(1 << 20, 40 + i) for i in range(3)] + [datagen.sparse(512, 300)]
    d = _Dev(texts)
    plain = engine.deflate_batch_device(d.in_ptrs(), d.lens, d.out_ptrs(), d.caps, level=6)
    want = [d.result(i, plain[i]) for i in range(d.n)]
    assert want[0] == oracle.compress(texts[0], 6)
    spec_plain = engine.counter("spec_streams")
    assert spec_plain >= 3
    d2 = _Dev(texts)
    lens = engine.deflate_writes_batch_device(d2.in_ptrs(), d2.lens, None, d2.out_ptrs(), d2.caps, level=6)
    assert [d2.result(i, lens[i]) for i in range(d2.n)] == want
    assert engine.counter("spec_streams") == spec_plain
    # lists for some: the others are single Writes inside a writes-batch
    d3 = _Dev(texts)
    rng = np.random.default_rng(1)
    lists = [None, _ends_of(len(texts[1]), 81920, rng), None, [len(texts[3])]]
    lens = engine.deflate_writes_batch_device(d3.in_ptrs(), d3.lens, lists, d3.out_ptrs(), d3.caps, level=6)
    assert engine.counter("spec_streams") >= 2, "the single-Write streams of a writes-batch left the speculative walk"
    for i in (0, 2, 3):
        assert d3.result(i, lens[i]) == want[i], i
    assert d3.result(1, lens[1]) == oracle.compress(texts[1], 6, chunks=_sizes(lists[1]))


def test_one_undersized_output_fails_that_stream_only(engine, oracle):
    rng = np.random.default_rng(3)
    datas = [oracle_binding.corpus("sum"), oracle_binding.corpus("kennedy.xls"), oracle_binding.corpus("cp.html")]
    lists = [_ends_of(len(datas[0]), 4000, rng), _ends_of(len(datas[1]), 81920, rng), _ends_of(len(datas[2]), ("r", 100, 3000), rng)]
    d = _Dev(datas, caps=[deflate_bound(len(datas[0])), 100, deflate_bound(len(datas[2]))])
    for level in (1, 6):
        rc, lens, status = engine.deflate_writes_batch_device(d.in_ptrs(), d.lens, lists, d.out_ptrs(), d.caps, level=level, return_status=True)
        assert rc == ZS_BUF_ERROR and status == [ZS_OK, ZS_BUF_ERROR, ZS_OK], (level, rc, status, engine.last_error())
        for i in (0, 2):
            assert d.result(i, lens[i]) == oracle.compress(datas[i], level, chunks=_sizes(lists[i])), (level, i)
        assert bytes(d.d_out[1][100:164].cpu().numpy()) == b"\xEE" * 64, "the short buffer was written beyond its capacity"


def test_a_malformed_list_fails_the_whole_call_before_any_device_work(engine):
    datas = [datagen.english(100000, 1), datagen.english(100000, 2)]
    d = _Dev(datas)
    L = engine._lib
    P64 = ctypes.POINTER(ctypes.c_int64)
    VP, I64, I32 = ctypes.c_void_p * 2, ctypes.c_int64 * 2, ctypes.c_int * 2
    good = (ctypes.c_int64 * 2)(50000, 100000)
    for bad in ((60000, 50000, 100000), (50000, 99999), (50000, 100001), (-1, 100000)):
        arr = (ctypes.c_int64 * len(bad))(*bad)
        olen, st = I64(7, 7), I32(7, 7)
        rc = L.zs_deflate_writes_batch_device(engine.handle, 2, VP(*d.in_ptrs()), I64(*d.lens), (P64 * 2)(ctypes.cast(good, P64), ctypes.cast(arr, P64)),
                                              I64(2, len(bad)), VP(*d.out_ptrs()), I64(*d.caps), olen, st, 6, 0, 0, None)
        assert rc == -2 and engine.last_error() == "stream error", (bad, rc, engine.last_error())
        import torch
        torch.cuda.synchronize()
        assert bytes(d.d_out[0][:64].cpu().numpy()) == b"\xEE" * 64, "stream 0 was written although stream 1's list is malformed"


def test_a_list_of_one_end_or_none_is_one_write_in_the_batch_and_in_the_single_call(engine, oracle):
    """The edge where the two entries' argument rules meet (zsgpu.h): n_writes[i] <= 0 and a one-end list are one Write in the
    batch; a one-end list is still checked against in_len[i]; zs_deflate_writes_device has no "no list" and rejects
    n_writes == 0 for a non-empty input, and takes the one-end list with the batch's bytes."""
    data = oracle_binding.corpus("cp.html")
    want = oracle.compress(data, 6)
    n = len(data)
    d = _Dev([data, data, data])
    L = engine._lib
    P64 = ctypes.POINTER(ctypes.c_int64)
    VP, I64, I32 = ctypes.c_void_p * 3, ctypes.c_int64 * 3, ctypes.c_int * 3
    one = (ctypes.c_int64 * 1)(n)
    lists = (P64 * 3)(ctypes.cast(one, P64), ctypes.cast(one, P64), P64())
    for counts in ((1, 0, 0), (1, -3, 5)):  # (stream 1: a pointer with no ends; stream 2: a count with no pointer)
        olen, st = I64(), I32(7, 7, 7)
        rc = L.zs_deflate_writes_batch_device(engine.handle, 3, VP(*d.in_ptrs()), I64(*d.lens), lists, I64(*counts), VP(*d.out_ptrs()), I64(*d.caps),
                                              olen, st, 6, 0, 0, None)
        assert rc == 0 and list(st) == [0, 0, 0], (counts, rc, engine.last_error())
        assert [d.result(i, olen[i]) for i in range(3)] == [want] * 3, counts
    short = (ctypes.c_int64 * 1)(n - 1)
    olen, st = I64(), I32()
    rc = L.zs_deflate_writes_batch_device(engine.handle, 3, VP(*d.in_ptrs()), I64(*d.lens), (P64 * 3)(ctypes.cast(short, P64), P64(), P64()), I64(1, 0, 0),
                                          VP(*d.out_ptrs()), I64(*d.caps), olen, st, 6, 0, 0, None)
    assert rc == -2 and engine.last_error() == "stream error"
    d1 = _Dev([data])
    o1 = ctypes.c_int64(0)
    args = (ctypes.c_void_p(d1.out_ptrs()[0]), d1.caps[0], ctypes.byref(o1), 6, 0, 0, None)
    assert L.zs_deflate_writes_device(engine.handle, ctypes.c_void_p(d1.in_ptrs()[0]), n, one, 0, *args) == -2
    assert L.zs_deflate_writes_device(engine.handle, ctypes.c_void_p(d1.in_ptrs()[0]), n, short, 1, *args) == -2
    assert L.zs_deflate_writes_device(engine.handle, ctypes.c_void_p(d1.in_ptrs()[0]), n, one, 1, *args) == 0
    assert d1.result(0, o1.value) == want


def test_a_writes_batch_larger_than_the_device_runs_in_sub_batches(engine, oracle):
    """As test_a_batch_larger_than_the_device_runs_in_sub_batches, over device pointers: 384 streams of 64 MiB -- 24 GiB of
    input, ~19 bytes of workspace per input byte -- do not fit one run of the pipeline.  The inputs are two device buffers
    passed again and again (text in 81 920-byte Writes, zeros without a list); every stream has an output buffer of its own.
    The call splits itself; the bytes are those of the two streams alone, which are the oracle's (a 4 MiB prefix compared,
    the whole stream by its inflation)."""
    import torch
    size = 64 << 20
    rng = np.random.default_rng(0)
    text, zeros = datagen.english(size, 77), bytes(size)
    ends = _ends_of(size, 81920, rng)
    one_text, one_zero = _alone(engine, text, ends, 6, 0), _alone(engine, zeros, None, 6, 0)
    assert zlib.decompress(one_text) == text and zlib.decompress(one_zero) == zeros
    pre = 4 << 20
    assert _alone(engine, text[:pre], _ends_of(pre, 81920, rng), 6, 0) == oracle.compress(text[:pre], 6, chunks=_sizes(_ends_of(pre, 81920, rng)))
    d_text = torch.frombuffer(bytearray(text) + bytearray(64), dtype=torch.uint8).cuda()
    d_zero = torch.zeros(size + 64, dtype=torch.uint8, device="cuda")
    n = 384
    is_text = [i % 32 < 7 for i in range(n)]  # 84 text streams among the 384
    caps = [deflate_bound(size) if t else 1 << 20 for t in is_text]
    outs = [torch.empty(c, dtype=torch.uint8, device="cuda") for c in caps]
    torch.cuda.synchronize()
    arr = (ctypes.c_int64 * len(ends))(*ends)
    rc, lens, status = engine.deflate_writes_batch_device([(d_text if t else d_zero).data_ptr() for t in is_text], [size] * n,
                                                          [arr if t else None for t in is_text], [o.data_ptr() for o in outs], caps, level=6,
                                                          return_status=True)
    assert rc == 0 and all(x == 0 for x in status), (rc, engine.last_error())
    for i in range(n):
        assert lens[i] == len(one_text if is_text[i] else one_zero), i
    for i in list(range(0, n, 37)) + [n - 1]:
        assert outs[i][:lens[i]].cpu().numpy().tobytes() == (one_text if is_text[i] else one_zero), i


# ---------------------------------------------------------------- 2. the filter of a batch of images
def _paeth_np(left, up, ul):
    p = left + up - ul
    pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
    return np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))


def _filter_reference(img, row_bytes, height, bpp, ftype):
    """PNG specification 9.2 in numpy -> height * (row_bytes + 1) bytes.  Adaptive (5): per row the filter with the smallest sum
    of the filtered bytes' absolute values read as signed, the first one on ties."""
    a = np.frombuffer(img, dtype=np.uint8).reshape(height, row_bytes).astype(np.int32)
    left, up, ul = np.zeros_like(a), np.zeros_like(a), np.zeros_like(a)
    if row_bytes > bpp:
        left[:, bpp:] = a[:, :-bpp]
        ul[1:, bpp:] = a[:-1, :-bpp]
    up[1:] = a[:-1]
    cands = [a, a - left, a - up, a - ((left + up) >> 1), a - _paeth_np(left, up, ul)]
    cands = [(c & 0xFF).astype(np.uint8) for c in cands]
    out = np.empty((height, row_bytes + 1), dtype=np.uint8)
    if ftype == 5:
        sums = np.stack([np.abs(c.view(np.int8).astype(np.int32)).sum(axis=1) for c in cands])
        pick = sums.argmin(axis=0)  # (the first minimum)
    else:
        pick = np.full(height, ftype)
    out[:, 0] = pick
    for f in range(5):
        rows = pick == f
        out[rows, 1:] = cands[f][rows]
    return out.tobytes()


def _images(seed=6):
    """(pixels, row_bytes, height, bpp, filter): sizes, bpp 1 / 3 / 4 / 8 and filters 0-5 mixed; widths that are no multiple of bpp;
    one image a single row, one a single byte wide, flat images whose adaptive sums tie, rows past what the kernel stages."""
    rng = np.random.default_rng(seed)

    def noisy(rb, h):
        grad = (np.add.outer(np.arange(h) * 3, np.arange(rb)) % 253).astype(np.uint8)
        return (grad + rng.integers(0, 4, grad.shape, dtype=np.uint8)).astype(np.uint8).tobytes()

    imgs = [(datagen.sparse(512, 64), 2048, 64, 4, 5), (noisy(333 * 4, 97), 333 * 4, 97, 4, 5), (noisy(333 * 4, 97), 333 * 4, 97, 3, 4),
            (bytes(rng.integers(0, 256, 77 * 5, dtype=np.uint8)), 77, 5, 1, 5), (noisy(1001, 1), 1001, 1, 3, 5), (noisy(1, 130), 1, 130, 1, 5),
            (noisy(7, 9), 7, 9, 8, 5), (bytes(300 * 40), 300, 40, 4, 5), (bytes([7]) * (64 * 33), 64, 33, 8, 5), (noisy(16384, 5), 16384, 5, 8, 5),
            (noisy(16385, 4), 16385, 4, 4, 5), (noisy(40001, 3), 40001, 3, 3, 5), (noisy(15, 1), 15, 1, 8, 3)]
    for f in range(6):
        for bpp in (1, 3, 4, 8):
            rb = int(rng.integers(1, 700))
            imgs.append((noisy(rb, int(rng.integers(1, 50))), rb, 0, bpp, f))
    return [(p, rb, len(p) // rb, bpp, f) for p, rb, _, bpp, f in imgs]


def _dev_images(imgs, odd_addresses=False):
    import torch
    # (odd_addresses: every image 1, 2, 3 ... bytes into its allocation, rows and outputs unaligned)
    d_px = [torch.frombuffer(bytearray(i % 16 if odd_addresses else 0) + bytearray(p) + bytearray(16), dtype=torch.uint8).cuda() for i, (p, *_) in enumerate(imgs)]
    d_f = [torch.full((h * (rb + 1) + 32,), 0xEE, dtype=torch.uint8, device="cuda") for _, rb, h, _, _ in imgs]
    torch.cuda.synchronize()
    off = [i % 16 if odd_addresses else 0 for i in range(len(imgs))]
    return d_px, d_f, off


@pytest.mark.parametrize("odd_addresses", [False, True])
def test_filter_batch_is_the_specification_and_n_single_calls(engine, odd_addresses):
    import torch
    from zlibstream_amd import png_filter_batch_device, png_filter_device
    imgs = _images()
    d_px, d_f, off = _dev_images(imgs, odd_addresses)
    png_filter_batch_device(engine, [t.data_ptr() + o for t, o in zip(d_px, off)], [rb for _, rb, _, _, _ in imgs], [h for _, _, h, _, _ in imgs],
                            [b for _, _, _, b, _ in imgs], [f for *_, f in imgs], [t.data_ptr() + (3 * o) % 7 for t, o in zip(d_f, off)])
    for i, (p, rb, h, bpp, f) in enumerate(imgs):
        n, o = h * (rb + 1), (3 * off[i]) % 7
        got = d_f[i][o:o + n].cpu().numpy().tobytes()
        assert got == _filter_reference(p, rb, h, bpp, f), "image %d: %d x %d, bpp %d, filter %d" % (i, rb, h, bpp, f)
        assert bytes(d_f[i][o + n:o + n + 16].cpu().numpy()) == b"\xEE" * 16 and bytes(d_f[i][:o].cpu().numpy()) == b"\xEE" * o, "image %d: written outside its rows" % i
        d_one = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        png_filter_device(engine, d_px[i].data_ptr() + off[i], rb, h, bpp, f, d_one.data_ptr())
        assert d_one.cpu().numpy().tobytes() == got, "image %d: the batch differs from the single call" % i


def test_filter_batch_without_its_lds_staging_is_the_specification(engine, monkeypatch):
    """ZS_PNG_NO_STAGE=1 (read at every call): every row takes the loads that rows above 16 KiB always take."""
    from zlibstream_amd import png_filter_batch_device
    monkeypatch.setenv("ZS_PNG_NO_STAGE", "1")
    imgs = _images()
    d_px, d_f, _ = _dev_images(imgs)
    png_filter_batch_device(engine, [t.data_ptr() for t in d_px], [rb for _, rb, _, _, _ in imgs], [h for _, _, h, _, _ in imgs],
                            [b for _, _, _, b, _ in imgs], [f for *_, f in imgs], [t.data_ptr() for t in d_f])
    for i, (p, rb, h, bpp, f) in enumerate(imgs):
        n = h * (rb + 1)
        assert d_f[i][:n].cpu().numpy().tobytes() == _filter_reference(p, rb, h, bpp, f), "image %d: %d x %d, bpp %d, filter %d" % (i, rb, h, bpp, f)
        assert bytes(d_f[i][n:n + 16].cpu().numpy()) == b"\xEE" * 16, "image %d: written outside its rows" % i


def test_filter_batch_of_more_rows_than_one_launch_holds(engine):
    """A grid holds fewer than 2^32 threads, so a call of more than 2^23 rows is several launches: one image a byte wide and
    2^23 + 5 rows high (its rows on both sides of the seam), and a small one behind it whose rows all lie in the second launch."""
    from zlibstream_amd import png_filter_batch_device
    rng = np.random.default_rng(31)
    tall = bytes(rng.integers(0, 256, (1 << 23) + 5, dtype=np.uint8))
    imgs = [(tall, 1, len(tall), 1, 5), (bytes(rng.integers(0, 256, 40 * 9, dtype=np.uint8)), 40, 9, 4, 5)]
    d_px, d_f, _ = _dev_images(imgs)
    png_filter_batch_device(engine, [t.data_ptr() for t in d_px], [1, 40], [len(tall), 9], [1, 4], [5, 5], [t.data_ptr() for t in d_f])
    for i, (p, rb, h, bpp, f) in enumerate(imgs):
        got = d_f[i][:h * (rb + 1)].cpu().numpy()
        want = np.frombuffer(_filter_reference(p, rb, h, bpp, f), dtype=np.uint8)
        assert np.array_equal(got, want), "image %d: first difference at byte %d" % (i, int(np.argmax(got != want)))


def test_filter_batch_on_the_callers_stream(engine):
    import torch
    from zlibstream_amd import png_filter_batch_device
    imgs = _images(seed=8)[:12]
    d_px, d_f, _ = _dev_images(imgs)
    s = torch.cuda.Stream()
    png_filter_batch_device(engine, [t.data_ptr() for t in d_px], [rb for _, rb, _, _, _ in imgs], [h for _, _, h, _, _ in imgs],
                            [b for _, _, _, b, _ in imgs], [f for *_, f in imgs], [t.data_ptr() for t in d_f], stream=s.cuda_stream)
    s.synchronize()
    for i, (p, rb, h, bpp, f) in enumerate(imgs):
        assert d_f[i][:h * (rb + 1)].cpu().numpy().tobytes() == _filter_reference(p, rb, h, bpp, f), i


# ---------------------------------------------------------------- 3. pixels -> IDAT payloads
def _idat_images():
    rng = np.random.default_rng(12)
    imgs = []
    for i in range(64):
        kind = i % 4
        w, h = int(rng.integers(20, 200)), int(rng.integers(1, 160))
        if i == 5:
            w, h = 700, 300  # one image whose rows cross several window ends
        bpp = (4, 3, 1, 8)[kind]
        if kind == 0:
            px = datagen.sparse(w, h, y0=i)
        else:
            grad = (np.add.outer(np.arange(h) * (i % 5), np.arange(w * bpp)) % 251).astype(np.uint8)
            px = (grad + rng.integers(0, 3, grad.shape, dtype=np.uint8)).astype(np.uint8).tobytes()
        imgs.append((px, w * bpp, h, bpp, (5, 5, 4, 1, 0, 2, 3)[i % 7]))
    return imgs


@pytest.mark.parametrize("rows_per_write", [0, 1, 7])
@pytest.mark.parametrize("level", [1, 6])
def test_idat_batch_is_the_oracle_on_the_filtered_rows_and_decodes_to_the_pixels(engine, oracle, level, rows_per_write):
    """64 images in one call: every stream is the oracle's on (the numpy-filtered rows, Writes of rows_per_write rows), and
    zs_inflate_batch_device plus zs_png_unfilter_batch_device give the pixels back without leaving the device.  The second
    level runs on the caller's stream."""
    import torch
    from zlibstream_amd import png_idat_batch_device, png_unfilter_batch_device
    imgs = _idat_images()
    n = len(imgs)
    d_px, _, _ = _dev_images(imgs)
    flen = [h * (rb + 1) for _, rb, h, _, _ in imgs]
    caps = [deflate_bound(x) + 64 * h for x, (_, _, h, _, _) in zip(flen, imgs)]
    d_z = [torch.full((c,), 0xEE, dtype=torch.uint8, device="cuda") for c in caps]
    torch.cuda.synchronize()
    s = torch.cuda.Stream() if level == 6 else None
    lens = png_idat_batch_device(engine, [t.data_ptr() for t in d_px], [rb for _, rb, _, _, _ in imgs], [h for _, _, h, _, _ in imgs],
                                 [b for _, _, _, b, _ in imgs], [f for *_, f in imgs], [t.data_ptr() for t in d_z], caps,
                                 rows_per_write=rows_per_write, level=level, stream=s.cuda_stream if s else None)
    for i, (px, rb, h, bpp, f) in enumerate(imgs):
        rows = _filter_reference(px, rb, h, bpp, f)
        k = rows_per_write if rows_per_write else h
        chunks = [min(k, h - y) * (rb + 1) for y in range(0, h, k)]
        want = oracle.compress(rows, level, 0, chunks=chunks if len(chunks) > 1 else None)
        assert d_z[i][:lens[i]].cpu().numpy().tobytes() == want, "level %d, %d rows a Write, image %d (%d x %d, bpp %d, filter %d)" % (level, rows_per_write, i, rb, h, bpp, f)
    # and back, on the device
    d_rows = [torch.zeros(x, dtype=torch.uint8, device="cuda") for x in flen]
    d_back = [torch.zeros(h * rb, dtype=torch.uint8, device="cuda") for _, rb, h, _, _ in imgs]
    torch.cuda.synchronize()
    out_lens = engine.inflate_batch_device([t.data_ptr() for t in d_z], lens, [t.data_ptr() for t in d_rows], flen)
    assert out_lens == flen
    st = png_unfilter_batch_device(engine, [t.data_ptr() for t in d_rows], [rb for _, rb, _, _, _ in imgs], [h for _, _, h, _, _ in imgs],
                                   [b for _, _, _, b, _ in imgs], [t.data_ptr() for t in d_back])
    assert st == [0] * n
    for i, (px, *_rest) in enumerate(imgs):
        assert d_back[i].cpu().numpy().tobytes() == px, i


def test_writes_batch_on_the_callers_stream(engine, oracle):
    import torch
    rng = np.random.default_rng(21)
    datas = [datagen.english(300000, 50 + i) for i in range(4)]
    lists = [_ends_of(len(x), ("r", 500, 70000), rng) for x in datas]
    d = _Dev(datas)
    s = torch.cuda.Stream()
    for level in (2, 6):
        lens = engine.deflate_writes_batch_device(d.in_ptrs(), d.lens, lists, d.out_ptrs(), d.caps, level=level, stream=s.cuda_stream)
        for i in range(4):
            assert d.result(i, lens[i]) == oracle.compress(datas[i], level, chunks=_sizes(lists[i])), (level, i)
