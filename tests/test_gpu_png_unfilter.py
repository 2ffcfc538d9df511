"""PNG scanline reconstruction on the device (zs_png_unfilter_device / zs_png_unfilter_batch_device, kernel KU): against a
pure-Python restatement of PNG specification 9.2, as the inverse of the forward filter kernel, behind deflate and inflate
without a host copy, at the edges of the kernel's bands and workgroups, per segment count, as a batch with bad images in
it, and on a caller's stream.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

from zlibstream_amd import datagen, deflate_bound

pytestmark = pytest.mark.gpu

ZS_OK, ZS_DATA_ERROR = 0, -3


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def _unfilter_reference(filtered, row_bytes, height, bpp):
    """PNG specification 9.2, byte by byte: Recon(x) = Filt(x) + f(Recon(a), Recon(b), Recon(c)) mod 256."""
    out = bytearray(row_bytes * height)
    prior = bytes(row_bytes)
    for y in range(height):
        base = y * (row_bytes + 1)
        ft = filtered[base]
        row = bytearray(filtered[base + 1:base + 1 + row_bytes])
        for i in range(row_bytes):
            a = row[i - bpp] if i >= bpp else 0
            b = prior[i]
            c = prior[i - bpp] if i >= bpp else 0
            if ft == 1:
                row[i] = (row[i] + a) & 255
            elif ft == 2:
                row[i] = (row[i] + b) & 255
            elif ft == 3:
                row[i] = (row[i] + ((a + b) >> 1)) & 255
            elif ft == 4:
                row[i] = (row[i] + _paeth(a, b, c)) & 255
        out[y * row_bytes:(y + 1) * row_bytes] = row
        prior = bytes(row)
    return bytes(out)


def _random_filtered(rng, row_bytes, height, types):
    """height rows of a type byte and row_bytes random bytes; types: one value, or a callable of the row number."""
    f = rng.integers(0, 256, (height, row_bytes + 1), dtype=np.uint8)
    f[:, 0] = [types(y) if callable(types) else types for y in range(height)]
    return f


def _cuda(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).copy()).cuda()


def _unfilter(engine, d_in, row_bytes, height, bpp):
    import torch
    from zlibstream_amd import png_unfilter_device
    d_out = torch.full((row_bytes * height,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch filled it on its own stream; the engine's stream does not wait for that one
    png_unfilter_device(engine, d_in.data_ptr(), row_bytes, height, bpp, d_out.data_ptr())
    return d_out


def _filter(engine, d_img, row_bytes, height, bpp, ftype):
    import torch
    from zlibstream_amd import png_filter_device
    d_f = torch.zeros(height * (row_bytes + 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (as in _unfilter)
    png_filter_device(engine, d_img.data_ptr(), row_bytes, height, bpp, ftype, d_f.data_ptr())
    return d_f


# ---------------------------------------------------------------- the specification, restated
@pytest.mark.parametrize("bpp", [1, 2, 3, 4, 6, 8])
def test_spec_parity_on_small_images(engine, bpp):
    """Every fixed type and random types per row; widths that are and are not a multiple of bpp; one column; one row."""
    rng = np.random.default_rng(100 + bpp)
    shapes = [(37 * bpp, 41), (37 * bpp + (bpp > 1), 29), (130 * bpp + bpp // 2, 70), (bpp, 150), (1, 90), (301 * bpp, 1), (64 * bpp, 64)]
    for row_bytes, height in shapes:
        for types in (0, 1, 2, 3, 4, lambda y: int(rng.integers(0, 5))):
            f = _random_filtered(rng, row_bytes, height, types)
            got = _unfilter(engine, _cuda(f), row_bytes, height, bpp).cpu().numpy().tobytes()
            want = _unfilter_reference(f.tobytes(), row_bytes, height, bpp)
            assert got == want, (bpp, row_bytes, height, types if not callable(types) else "random")


def test_spec_parity_on_a_150_kb_image(engine):
    rng = np.random.default_rng(7)
    row_bytes, height, bpp = 4 * 187 + 3, 200, 4
    f = _random_filtered(rng, row_bytes, height, lambda y: int(rng.integers(0, 5)))
    got = _unfilter(engine, _cuda(f), row_bytes, height, bpp).cpu().numpy().tobytes()
    assert got == _unfilter_reference(f.tobytes(), row_bytes, height, bpp)


# ---------------------------------------------------------------- the inverse of the forward kernel
def _forward_test_images():
    """The four images of test_png_filter_kernel_and_the_deflate_of_its_rows."""
    rng = np.random.default_rng(4)
    w, h = 333, 97
    grad = (np.add.outer(np.arange(h), np.arange(w * 4)) % 251).astype(np.uint8)
    noisy = (grad + rng.integers(0, 3, grad.shape, dtype=np.uint8)).astype(np.uint8)
    return ((datagen.sparse(512, 256), 2048, 256, 4), (noisy.tobytes(), w * 4, h, 4), (noisy.tobytes(), w * 4, h, 3),
            (bytes(rng.integers(0, 256, 77 * 5, dtype=np.uint8)), 77, 5, 1))


def _noisy_gradient(width, height, seed):
    rng = np.random.default_rng(seed)
    grad = (np.add.outer(np.arange(height) * 3, np.arange(width)) % 253).astype(np.uint8)
    return (grad + rng.integers(0, 4, grad.shape, dtype=np.uint8)).astype(np.uint8)


@pytest.mark.parametrize("ftype", [0, 1, 2, 3, 4, 5])
def test_round_trip_with_the_forward_kernel(engine, ftype):
    """png_unfilter(png_filter(img, f)) == img, compared on the device."""
    import torch
    images = list(_forward_test_images())
    images.append((datagen.sparse(3500, 3500), 3500 * 4, 3500, 4))  # the reference's benchmark image, as RGBA
    images.append((_noisy_gradient(4096, 4096, 11).tobytes(), 4096, 4096, 1))
    for img, row_bytes, height, bpp in images:
        assert len(img) == row_bytes * height
        d_img = torch.frombuffer(bytearray(img), dtype=torch.uint8).cuda()
        d_f = _filter(engine, d_img, row_bytes, height, bpp, ftype)
        d_back = _unfilter(engine, d_f, row_bytes, height, bpp)
        assert torch.equal(d_back, d_img), (ftype, row_bytes, height, bpp)


def test_whole_decode_path_stays_in_hbm(engine):
    """pixels -> adaptive filter -> deflate level 6 -> inflate -> unfilter == pixels; only lengths cross to the host."""
    import torch
    for img, row_bytes, height, bpp in ((datagen.sparse(1024, 768), 4096, 768, 4), (_noisy_gradient(999 * 3, 500, 3).tobytes(), 999 * 3, 500, 3)):
        d_img = torch.frombuffer(bytearray(img), dtype=torch.uint8).cuda()
        d_f = _filter(engine, d_img, row_bytes, height, bpp, 5)
        cap = deflate_bound(d_f.numel())
        d_z = torch.empty(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        zlen = engine.deflate_batch_device([d_f.data_ptr()], [d_f.numel()], [d_z.data_ptr()], [cap], level=6)[0]
        d_idat = torch.zeros(d_f.numel(), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert engine.inflate_batch_device([d_z.data_ptr()], [zlen], [d_idat.data_ptr()], [d_idat.numel()]) == [d_f.numel()]
        d_back = _unfilter(engine, d_idat, row_bytes, height, bpp)
        assert torch.equal(d_back, d_img), (row_bytes, height, bpp)


# ---------------------------------------------------------------- the kernel's own edges
def _numpy_reference(f, row_bytes, height, bpp):
    """The plain loop's result as an array (to compare on the device)."""
    return np.frombuffer(_unfilter_reference(f.tobytes(), row_bytes, height, bpp), dtype=np.uint8)


@pytest.mark.parametrize("ftype", [3, 4])
def test_band_and_workgroup_edges(engine, ftype):
    """One segment (every row Average, or every row Paeth) whose height sits on the edges of a 64-row band and of the rows a
    workgroup has in flight, and whose width sits on the edges of a 64-pixel chunk."""
    import torch
    rng = np.random.default_rng(ftype)
    cases = [(4, 23, h) for h in (1, 63, 64, 65, 1023, 1024, 1025, 2049)]
    cases += [(bpp, wpx, h) for bpp in (1, 4, 8) for wpx in (1, 63, 64, 65) for h in (65, 300)]
    cases += [(3, 129, 520), (6, 70, 200)]
    for bpp, width_px, height in cases:
        row_bytes = width_px * bpp
        f = _random_filtered(rng, row_bytes, height, ftype)
        got = _unfilter(engine, _cuda(f), row_bytes, height, bpp)
        assert engine.counter("png_segments") == 1
        want = torch.from_numpy(_numpy_reference(f, row_bytes, height, bpp).copy()).cuda()
        assert torch.equal(got, want), (ftype, bpp, width_px, height)


def test_segment_counts(engine):
    """A segment starts at row 0 and at every None or Sub row: `height` of them for all-Sub, one for all-Paeth,
    ceil(height / 100) when every 100th row is None and the rest Paeth -- and the pixels are right in each case."""
    import torch
    rng = np.random.default_rng(12)
    row_bytes, height, bpp = 4 * 75, 730, 4
    for types, segments in ((1, height), (4, 1), (lambda y: 0 if y % 100 == 0 else 4, -(-height // 100))):
        f = _random_filtered(rng, row_bytes, height, types)
        got = _unfilter(engine, _cuda(f), row_bytes, height, bpp)
        assert engine.counter("png_segments") == segments
        want = torch.from_numpy(_numpy_reference(f, row_bytes, height, bpp).copy()).cuda()
        assert torch.equal(got, want), segments


# ---------------------------------------------------------------- many images per call
def test_batch_with_two_bad_images(engine):
    import torch
    from zlibstream_amd import png_unfilter_batch_device
    rng = np.random.default_rng(5)
    shapes = [(4, 100, 80), (1, 333, 17), (3, 3 * 65 + 1, 130), (8, 8 * 40, 66), (2, 2 * 200, 5), (4, 4 * 64, 64), (6, 6 * 33, 90), (1, 1, 200),
              (4, 4 * 300 + 2, 1), (2, 127, 129), (3, 3, 70), (8, 8 * 129, 30)]
    fs = [_random_filtered(rng, rb, h, lambda y: int(rng.integers(0, 5))) for _, rb, h in shapes]
    bad_mid, bad_first = 3, 9
    fs[bad_mid][31, 0] = 5
    fs[bad_mid][50, 0] = 200
    fs[bad_first][0, 0] = 255
    d_in = [_cuda(f) for f in fs]
    d_out = [torch.full((rb * h,), 0xEE, dtype=torch.uint8, device="cuda") for _, rb, h in shapes]
    torch.cuda.synchronize()
    args = ([t.data_ptr() for t in d_in], [rb for _, rb, _ in shapes], [h for _, _, h in shapes], [bpp for bpp, _, _ in shapes],
            [t.data_ptr() for t in d_out])
    status = png_unfilter_batch_device(engine, *args)
    assert status == [ZS_DATA_ERROR if i in (bad_mid, bad_first) else ZS_OK for i in range(len(shapes))]
    assert engine.last_error() == "data error: image %d: row 31 has a filter type above 4" % bad_mid
    for i, (bpp, rb, h) in enumerate(shapes):
        if i not in (bad_mid, bad_first):
            assert d_out[i].cpu().numpy().tobytes() == _unfilter_reference(fs[i].tobytes(), rb, h, bpp), i
    # the C entry point itself returns the first failing image's code; the other bad image alone names its own row
    n = len(shapes)
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    st = I32()
    rc = engine._lib.zs_png_unfilter_batch_device(engine.handle, n, VP(*args[0]), I64(*args[1]), I64(*args[2]), I32(*args[3]), VP(*args[4]), st, None)
    assert rc == ZS_DATA_ERROR and list(st) == status
    assert engine._lib.zs_png_unfilter_batch_device(engine.handle, 0, None, None, None, None, None, None, None) == ZS_OK
    assert png_unfilter_batch_device(engine, [], [], [], [], []) == []
    bpp, rb, h = shapes[bad_first]
    from zlibstream_amd import ZlibStreamException, png_unfilter_device
    with pytest.raises(ZlibStreamException) as ei:
        png_unfilter_device(engine, d_in[bad_first].data_ptr(), rb, h, bpp, d_out[bad_first].data_ptr())
    assert str(ei.value) == "png: data error: image 0: row 0 has a filter type above 4"


def test_on_the_callers_stream(engine):
    """Issued on a non-default stream behind the kernel that produces its input there: right when the call returns."""
    import torch
    row_bytes, height, bpp = 4 * 500, 300, 4
    img = _noisy_gradient(row_bytes, height, 21)
    d_img = torch.from_numpy(img.reshape(-1).copy()).cuda()
    d_f = torch.zeros(height * (row_bytes + 1), dtype=torch.uint8, device="cuda")
    d_out = torch.full((row_bytes * height,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    from zlibstream_amd import png_filter_device, png_unfilter_device
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        scratch = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):
            scratch = scratch @ scratch * 1e-3  # keeps the stream busy ahead of the filter kernel
        png_filter_device(engine, d_img.data_ptr(), row_bytes, height, bpp, 5, d_f.data_ptr(), stream=s.cuda_stream)
        png_unfilter_device(engine, d_f.data_ptr(), row_bytes, height, bpp, d_out.data_ptr(), stream=s.cuda_stream)
        got = d_out.cpu()  # (the call has synchronised the stream: no further wait)
    assert torch.equal(got, d_img.cpu())


def test_c_entry_points_reject_bad_arguments_with_a_real_context(engine):
    """The checks of the C entry points themselves (the Python layer raises before it reaches them): with a live context,
    bpp 0 or 9, row_bytes 0, height 0 or above 2^31 - 1, a null pointer array and a null entry return ZS_STREAM_ERROR, write
    nothing, and leave the context usable."""
    import torch
    L, h = engine._lib, engine.handle
    row_bytes, height, bpp = 40, 30, 4
    rng = np.random.default_rng(3)
    f = _random_filtered(rng, row_bytes, height, 4)
    d_in = _cuda(f)
    d_out = torch.full((row_bytes * height,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pin, pout = ctypes.c_void_p(d_in.data_ptr()), ctypes.c_void_p(d_out.data_ptr())
    VP, I64, I32 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_int * 1
    for rb, ht, bp in ((row_bytes, height, 0), (row_bytes, height, 9), (row_bytes, height, -1), (0, height, bpp), (-5, height, bpp),
                       (row_bytes, 0, bpp), (row_bytes, -1, bpp), (row_bytes, 1 << 31, bpp)):
        assert L.zs_png_unfilter_device(h, pin, rb, ht, bp, pout, None) == -2, (rb, ht, bp)
        st = I32(7)
        assert L.zs_png_unfilter_batch_device(h, 1, VP(pin), I64(rb), I64(ht), I32(bp), VP(pout), st, None) == -2, (rb, ht, bp)
        assert st[0] == -2
    assert L.zs_png_unfilter_device(h, None, row_bytes, height, bpp, pout, None) == -2
    assert L.zs_png_unfilter_device(h, pin, row_bytes, height, bpp, None, None) == -2
    assert L.zs_png_unfilter_batch_device(h, 1, None, I64(row_bytes), I64(height), I32(bpp), VP(pout), None, None) == -2
    assert L.zs_png_unfilter_batch_device(h, 1, VP(pin), None, I64(height), I32(bpp), VP(pout), None, None) == -2
    assert L.zs_png_unfilter_batch_device(h, 1, VP(pin), I64(row_bytes), None, I32(bpp), VP(pout), None, None) == -2
    assert L.zs_png_unfilter_batch_device(h, 1, VP(pin), I64(row_bytes), I64(height), None, VP(pout), None, None) == -2
    assert L.zs_png_unfilter_batch_device(h, 1, VP(pin), I64(row_bytes), I64(height), I32(bpp), None, None, None) == -2
    assert L.zs_png_unfilter_batch_device(h, -1, VP(pin), I64(row_bytes), I64(height), I32(bpp), VP(pout), None, None) == -2
    # one bad entry among good ones rejects the call before anything runs
    VP2, I642, I322 = ctypes.c_void_p * 2, ctypes.c_int64 * 2, ctypes.c_int * 2
    assert L.zs_png_unfilter_batch_device(h, 2, VP2(pin, pin), I642(row_bytes, row_bytes), I642(height, height), I322(bpp, 9), VP2(pout, pout),
                                          None, None) == -2
    assert L.zs_png_unfilter_batch_device(h, 2, VP2(pin, None), I642(row_bytes, row_bytes), I642(height, height), I322(bpp, bpp),
                                          VP2(pout, pout), None, None) == -2
    assert bool((d_out == 0xEE).all())
    assert L.zs_png_unfilter_device(h, pin, row_bytes, height, bpp, pout, None) == 0
    assert d_out.cpu().numpy().tobytes() == _unfilter_reference(f.tobytes(), row_bytes, height, bpp)
