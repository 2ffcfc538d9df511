"""The frame diff (zs_png_diff_batch_device, KD) and the crop (zs_png_crop_batch_device) on the device against their rules
restated on numpy arrays (tests/png_anim_read.py diff_ref; a slice).  One batch per format mixes canvas sizes, frame counts
(1 included), change patterns and pointer residues; every comparison is exact."""
import ctypes

import numpy as np
import pytest

from png_anim_read import RGBA8, RGBA16, diff_ref

pytestmark = pytest.mark.gpu

ZS_OK, ZS_STREAM_ERROR = 0, -2
# width x height: rows that end inside a group, cross a stretch's end (256 pixels of RGBA8, 128 of RGBA16), canvases whose size
# is no multiple of 16, and one with more waves (rows) than the 256 threads that fold a frame's records take at a time
SHAPES = ((1, 1), (1, 5), (3, 1), (5, 3), (261, 2), (257, 3), (129, 3), (5, 300))


def _px(fmt):
    return 8 if fmt == RGBA16 else 4


def patterns(w, h, fmt):
    """lists of (x, y, kind): 0 the whole pixel, 1 alpha only, 2 the low byte of a sample only, 3 a colour under alpha 0"""
    n = 16 // _px(fmt)
    out = [[]]
    out += [[(x, y, 0)] for y in (0, h - 1) for x in (0, w - 1)]
    out += [[(w // 2, 0, 0)], [(w // 2, h - 1, 0)], [(0, h // 2, 0)], [(w - 1, h // 2, 0)]]
    for x in (n - 1, n, 64 * n - 1, 64 * n):
        if x < w:
            out += [[(x, h // 2, 0)], [(x, h - 1, 1)]]
    out += [[(w // 2, h // 2, 1)], [(w // 3, h // 2, 2)], [(w - 1, 0, 3)], [(0, 0, 0), (w - 1, h - 1, 0)], [(w - 1, 0, 0), (0, h - 1, 0)]]
    return out


def make_anims(fmt):
    """-> a list of (n_frames, h, w, 4) arrays: per shape animations of 1, 2 and 3 frames and enough of 9 to use every pattern"""
    rng = np.random.default_rng(5100 + fmt)
    top = 65536 if fmt == RGBA16 else 256
    dt = np.uint16 if fmt == RGBA16 else np.uint8
    anims, under_zero = [], 0
    for w, h in SHAPES:
        pats = patterns(w, h, fmt)
        at = 0
        for nf in [1, 2, 3] + [9] * (-(-len(pats) // 8) + 1):
            c = rng.integers(0, top, (h, w, 4)).astype(dt)
            c[0, w - 1, 3] = 0  # (kind 3 changes the colour under this alpha)
            cv = [c]
            for f in range(1, nf):
                c = c.copy()
                for x, y, kind in pats[at % len(pats)]:
                    if kind == 0:
                        c[y, x] ^= np.array([1, 2, 4, 8 if c[y, x, 3] else 0], dtype=dt) << (f % 4)  # (an alpha of 0 stays: kind 3 needs it)
                    elif kind == 1:
                        c[y, x, 3] ^= 0x40
                    elif kind == 2:
                        c[y, x, 1] ^= 1  # (RGBA16: G's low byte)
                    else:
                        under_zero += int(c[y, x, 3] == 0)
                        c[y, x, 0] ^= 0x80
                at += 1
                cv.append(c)
            if nf == 3:
                cv[2] = cv[0].copy()  # A, B, A: frame 2 is B's change once more
            anims.append(np.stack(cv))
    assert under_zero >= len(SHAPES) // 2, "colour changes under alpha 0 are among the patterns"
    return anims


def place(anims, fmt):
    """the animations in one device buffer, animation k at a residue of (k * pixel size) % 16 -> (tensor, device pointers)"""
    import torch
    px = _px(fmt)
    offs, at = [], 0
    for k, a in enumerate(anims):
        at = (at + 15) // 16 * 16 + (k * px) % 16
        offs.append(at)
        at += a.nbytes
    host = np.full(at + 16, 0xEE, dtype=np.uint8)
    for o, a in zip(offs, anims):
        host[o:o + a.nbytes] = np.frombuffer(a.tobytes(), dtype=np.uint8)
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 16 == 0
    return t, [t.data_ptr() + o for o in offs]


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_the_rectangles_are_the_bounding_boxes_of_the_differing_pixels(engine, fmt):
    import torch
    from zlibstream_amd import png_diff_batch_device
    anims = make_anims(fmt)
    t, ptrs = place(anims, fmt)
    torch.cuda.synchronize()
    got = png_diff_batch_device(engine, ptrs, [a.shape[0] for a in anims], [a.shape[2] for a in anims], [a.shape[1] for a in anims], format=fmt)
    want = [diff_ref(a) for a in anims]
    assert {len(w) for w in want} == {1, 2, 3, 9} and {ptr % 16 for ptr in ptrs} == set(range(0, 16, _px(fmt)))
    assert any(r == (0, 0, 1, 1) for w in want for r in w[1:]), "the batch holds a frame without a change"
    for k, (a, g, w) in enumerate(zip(anims, got, want)):
        assert [(f["x"], f["y"], f["width"], f["height"]) for f in g] == w, (k, a.shape)
        assert all(f["dispose_op"] == 0 and f["blend_op"] == 0 for f in g)
    # the same call again, on a stream of the caller: the same rectangles (nothing depends on the run)
    s = torch.cuda.Stream()
    again = png_diff_batch_device(engine, ptrs, [a.shape[0] for a in anims], [a.shape[2] for a in anims], [a.shape[1] for a in anims], format=fmt, stream=s.cuda_stream)
    assert again == got


def test_the_diff_leaves_the_delay_and_data_fields_alone_and_checks_its_arguments(engine):
    import torch
    from zlibstream_amd import _native
    L = _native.lib()
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    t[2 * 5 * 3 * 4 + 7] = 1  # canvas 2 of a 5 x 3 animation: the alpha of pixel (1, 0)
    torch.cuda.synchronize()
    VP, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    frames = (_native.PngFrame * 3)()
    for f in frames:
        f.x = f.y = f.width = f.height = f.dispose_op = f.blend_op = 77
        f.delay_num, f.delay_den, f.data_bytes, f.n_chunks = 5, 6, 7, 8
    fp = (ctypes.POINTER(_native.PngFrame) * 1)(ctypes.cast(frames, ctypes.POINTER(_native.PngFrame)))

    def call(n=1, ctx=engine.handle, cv=(t.data_ptr(),), nf=(3,), w=(5,), h=(3,), fmt=RGBA8, out=fp):
        arr = lambda ty, v: None if v is None else (ty * len(v))(*v)
        return L.zs_png_diff_batch_device(ctx, n, arr(VP, cv), arr(I32, nf), arr(I64, w), arr(I64, h), fmt, out, None)

    for kw in (dict(ctx=None), dict(n=-1), dict(cv=None), dict(nf=None), dict(w=None), dict(h=None), dict(out=None), dict(cv=(None,)), dict(nf=(0,)), dict(w=(0,)),
               dict(w=(1 << 31,)), dict(h=(0,)), dict(h=(1 << 31,)), dict(fmt=2), dict(fmt=-1), dict(cv=(t.data_ptr() + 2,)), dict(fmt=RGBA16, cv=(t.data_ptr() + 4,)),
               dict(out=(ctypes.POINTER(_native.PngFrame) * 1)()), dict(w=(1 << 20,), h=(1 << 20,)),
               dict(n=2, nf=((1 << 31) - 1, 1), cv=(t.data_ptr(),) * 2, w=(5, 5), h=(3, 3), out=(ctypes.POINTER(_native.PngFrame) * 2)(fp[0], fp[0]))):
        assert call(**kw) == ZS_STREAM_ERROR, kw
        assert frames[1].x == 77 and frames[0].width == 77, kw
    assert call(n=0, cv=None, nf=None, w=None, h=None, out=None) == ZS_OK
    assert call() == ZS_OK
    assert [(f.x, f.y, f.width, f.height, f.dispose_op, f.blend_op) for f in frames] == [(0, 0, 5, 3, 0, 0), (0, 0, 1, 1, 0, 0), (1, 0, 1, 1, 0, 0)]
    assert all((f.delay_num, f.delay_den, f.data_bytes, f.n_chunks) == (5, 6, 7, 8) for f in frames)


CROP_IMAGE = (23, 7)
CROP_RECTS = ((0, 0, 23, 7), (0, 0, 1, 1), (22, 6, 1, 1), (0, 2, 9, 3), (14, 0, 9, 2), (3, 4, 17, 3), (5, 1, 1, 5), (22, 0, 1, 7), (2, 2, 13, 1), (1, 1, 21, 5))


@pytest.mark.parametrize("px", [4, 8])
def test_the_crop_at_every_pair_of_residues_with_guard_bytes(engine, px):
    """rectangles touching each edge, of width 1 and the whole image, every source and destination residue modulo 16, in one
    launch; the bytes between the outputs stay as they were"""
    import torch
    from zlibstream_amd import png_crop_batch_device
    rng = np.random.default_rng(5200 + px)
    iw, ih = CROP_IMAGE
    img = rng.integers(0, 256, (ih, iw, px), dtype=np.uint8)
    jobs, out_at = [], 64  # (source residue, 0, where the output begins, x, y, width, height)
    for sres in range(0, 16, px):
        for dres in range(0, 16, px):
            for x, y, w, h in CROP_RECTS:
                out_at = (out_at + 15) // 16 * 16 + 48 + dres  # (48 guard bytes and more between two outputs)
                jobs.append((sres, 0, out_at, x, y, w, h))
                out_at += w * h * px
    # one copy of the image per source residue, each in a block of its own
    blocks = {sres: k * ((img.nbytes + 31) // 16 * 16) + sres for k, sres in enumerate(range(0, 16, px))}
    src = np.full(max(blocks.values()) + img.nbytes + 16, 0xEE, dtype=np.uint8)
    for o in blocks.values():
        src[o:o + img.nbytes] = img.reshape(-1)
    want = np.full(out_at + 64, 0xEE, dtype=np.uint8)
    for sres, _, o, x, y, w, h in jobs:
        want[o:o + w * h * px] = img[y:y + h, x:x + w].reshape(-1)
    d_src, d_out = torch.from_numpy(src).cuda(), torch.full((len(want),), 0xEE, dtype=torch.uint8, device="cuda")
    assert d_src.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    png_crop_batch_device(engine, [d_src.data_ptr() + blocks[j[0]] for j in jobs], [iw] * len(jobs), [j[3] for j in jobs], [j[4] for j in jobs], [j[5] for j in jobs],
                          [j[6] for j in jobs], [d_out.data_ptr() + j[2] for j in jobs], pixel_bytes=px)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    assert d_src.cpu().numpy().tobytes() == src.tobytes()


def test_a_crop_of_more_rows_than_one_launch_holds(engine):
    """A launch of the flat-list kernels takes 2^25 rows, so a call of more is several launches, each with its first row: one
    image a pixel wide and 2^25 + 5 rows high (its rows on both sides of the seam), and a 7 x 9 rectangle of a 16 x 12 image
    behind it whose rows all lie in the second launch.  About 270 MB of device memory, compared there."""
    import torch
    from zlibstream_amd import png_crop_batch_device
    tall_h, guard = (1 << 25) + 5, 64
    gen = torch.Generator(device="cuda").manual_seed(5300)
    tall = torch.randint(0, 256, (tall_h, 1, 4), dtype=torch.uint8, device="cuda", generator=gen)
    small = torch.randint(0, 256, (12, 16, 4), dtype=torch.uint8, device="cuda", generator=gen)
    x, y, w, h = 5, 2, 7, 9
    outs = [torch.full((tall_h * 4 + guard,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((w * h * 4 + guard,), 0xEE, dtype=torch.uint8, device="cuda")]
    torch.cuda.synchronize()
    png_crop_batch_device(engine, [tall.data_ptr(), small.data_ptr()], [1, 16], [0, x], [0, y], [1, w], [tall_h, h], [t.data_ptr() for t in outs], pixel_bytes=4)
    torch.cuda.synchronize()
    for i, (out, want) in enumerate(zip(outs, (tall, small[y:y + h, x:x + w]))):
        n = want.numel()
        assert torch.equal(out[:n], want.reshape(-1)), "image %d" % i
        assert bool((out[n:] == 0xEE).all()), "image %d: written behind its rows" % i


def test_the_crop_checks_its_arguments(engine):
    import torch
    from zlibstream_amd import _native
    L = _native.lib()
    d_in, d_out = torch.zeros(4096, dtype=torch.uint8, device="cuda"), torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    VP, I64 = ctypes.c_void_p, ctypes.c_int64

    def call(n=1, ctx=engine.handle, src=(d_in.data_ptr(),), iw=(8,), x=(2,), y=(1,), w=(5,), h=(3,), px=4, out=(d_out.data_ptr(),)):
        arr = lambda ty, v: None if v is None else (ty * len(v))(*v)
        return L.zs_png_crop_batch_device(ctx, n, arr(VP, src), arr(I64, iw), arr(I64, x), arr(I64, y), arr(I64, w), arr(I64, h), px, arr(VP, out), None)

    for kw in (dict(ctx=None), dict(n=-1), dict(src=None), dict(iw=None), dict(x=None), dict(y=None), dict(w=None), dict(h=None), dict(out=None), dict(src=(None,)),
               dict(out=(None,)), dict(px=3), dict(px=16), dict(src=(d_in.data_ptr() + 2,)), dict(out=(d_out.data_ptr() + 2,)), dict(px=8, out=(d_out.data_ptr() + 4,)),
               dict(iw=(0,)), dict(iw=(1 << 31,)), dict(w=(0,)), dict(h=(0,)), dict(h=(1 << 31,)), dict(x=(-1,)), dict(y=(-1,)), dict(x=(4,)), dict(w=(9,))):
        assert call(**kw) == ZS_STREAM_ERROR, kw
    assert call(n=0, src=None, iw=None, x=None, y=None, w=None, h=None, out=None) == ZS_OK
    assert d_out.cpu().numpy().tobytes() == b"\xEE" * 4096
    assert call(x=(3,)) == ZS_OK  # x + width == in_width


def test_the_stage_timer_shows_the_diff_and_the_crop(engine):
    import torch
    from zlibstream_amd import png_crop_batch_device, png_diff_batch_device
    t = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    t[4000] = 1
    torch.cuda.synchronize()
    engine.set_profiling(True)
    try:
        png_diff_batch_device(engine, [t.data_ptr()], [3], [20], [10])
        diff = engine.stage_ms()
        png_crop_batch_device(engine, [t.data_ptr()], [20], [3], [2], [9], [5], [t.data_ptr() + 4096])
        crop = engine.stage_ms()
    finally:
        engine.set_profiling(False)
    assert diff.get("png_diff", 0) > 0 and crop.get("png_crop", 0) > 0, (diff, crop)
