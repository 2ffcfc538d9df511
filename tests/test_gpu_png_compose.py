"""The frames of animations composed into canvases on the device (zs_png_compose_batch_device, KM).  The reference is the numpy
restatement of the rules in include/zsgpu.h (tests/png_anim_ref.py compose_ref: frame by frame on a full canvas, the APNG
specification's integer OVER), which tests/test_png_anim_host.py anchors to Pillow; every comparison is exact."""
import ctypes

import numpy as np
import pytest

from png_anim_ref import BACKGROUND, NONE, OVER, PREVIOUS, RGBA8, RGBA16, SOURCE, compose_ref

pytestmark = pytest.mark.gpu

ZS_OK, ZS_STREAM_ERROR = 0, -2
GUARD = 64
PAIRS = [(d, b) for d in (NONE, BACKGROUND, PREVIOUS) for b in (SOURCE, OVER)]


def _px(fmt):
    return 8 if fmt == RGBA16 else 4


def _dtype(fmt):
    return "<u2" if fmt == RGBA16 else np.uint8


def pixels(rng, w, h, fmt):
    """random pixels, a third of them transparent, a third opaque"""
    top = 65535 if fmt == RGBA16 else 255
    a = rng.integers(0, top + 1, (h, w, 4)).astype(_dtype(fmt))
    kind = rng.integers(0, 3, (h, w))
    a[..., 3] = np.where(kind == 0, 0, np.where(kind == 1, top, a[..., 3]))
    return a


def frame(rng, fmt, x, y, w, h, dispose, blend):
    return dict(x=x, y=y, width=w, height=h, dispose_op=dispose, blend_op=blend, px=pixels(rng, w, h, fmt))


def run_compose(engine, anims, fmt, stream=None, residues=None):
    """one call over anims (dicts of w, h, frames) -> the canvases' bytes per animation.  Every frame's pixels lie in one
    buffer at pixel-aligned places of changing residue modulo 16; every output in a 0xEE-filled tensor of its own with GUARD
    bytes in front of it and behind it, both checked, at residues[i] modulo 16."""
    import torch
    from zlibstream_amd import png_compose_batch_device
    px = _px(fmt)
    blob, ptr_off, k = bytearray(), [], 0
    for a in anims:
        offs = []
        for f in a["frames"]:
            while len(blob) % 16 != (k * px) % 16:
                blob += b"\xCC"
            offs.append(len(blob))
            blob += np.ascontiguousarray(f["px"]).astype(_dtype(fmt)).tobytes()
            k += 1
        ptr_off.append(offs)
    d_px = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).cuda()
    assert d_px.data_ptr() % 16 == 0
    residues = residues or [0] * len(anims)
    sizes = [a["w"] * a["h"] * px * len(a["frames"]) for a in anims]
    d_out = [torch.full((GUARD + 16 + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for n in sizes]
    starts = [GUARD + (r - (t.data_ptr() + GUARD)) % 16 for t, r in zip(d_out, residues)]
    torch.cuda.synchronize()  # torch filled them on its own stream; the engine's stream does not wait for that one
    png_compose_batch_device(engine, [[d_px.data_ptr() + o for o in offs] for offs in ptr_off], [a["frames"] for a in anims], [a["w"] for a in anims],
                             [a["h"] for a in anims], [t.data_ptr() + s for t, s in zip(d_out, starts)], format=fmt, stream=stream)
    if stream is not None:
        torch.cuda.synchronize()
    got = []
    for t, s, n in zip(d_out, starts, sizes):
        b = t.cpu().numpy().tobytes()
        assert b[:s] == b"\xEE" * s and b[s + n:] == b"\xEE" * (len(b) - s - n), "bytes outside an output were written"
        got.append(b[s:s + n])
    return got


def check(engine, anims, fmt, **kw):
    got = run_compose(engine, anims, fmt, **kw)
    for a, g in zip(anims, got):
        want = b"".join(compose_ref(a["w"], a["h"], a["frames"], fmt))
        if g != want:
            n = a["w"] * a["h"] * _px(fmt)
            bad = [k for k in range(len(a["frames"])) if g[k * n:(k + 1) * n] != want[k * n:(k + 1) * n]]
            raise AssertionError("%dx%d: canvases %r differ" % (a["w"], a["h"], bad))
    return got


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_canvases_and_regions(engine, fmt):
    """1x1, 5x3, 67x4 and 261x2 (a second wave for the row, with a ragged end) in one call: the whole canvas, regions at x offsets
    0 .. 3, regions of 1x1 in the corners, regions touching the right and the bottom edge, the six dispose-blend pairs in turn"""
    rng = np.random.default_rng(8201 + fmt)
    anims = []
    for w, h in ((1, 1), (5, 3), (67, 4), (261, 2)):
        regions = [(0, 0, w, h)] + [(min(xo, w - 1), 0, max(1, (w - min(xo, w - 1)) // 2), h) for xo in range(4)]
        regions += [(0, 0, 1, 1), (w - 1, h - 1, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (w // 2, h // 2, w - w // 2, h - h // 2), (w // 3, 0, w - w // 3, 1),
                    (0, h - 1, w, 1), (0, 0, w, h)]
        frames = [frame(rng, fmt, x, y, fw, fh, *PAIRS[k % 6]) for k, (x, y, fw, fh) in enumerate(regions)]
        anims.append(dict(w=w, h=h, frames=frames))
    check(engine, anims, fmt)
    for a in anims:  # ... and one by one
        check(engine, [a], fmt)


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_every_dispose_blend_pair_and_previous_in_a_row(engine, fmt):
    rng = np.random.default_rng(8203 + fmt)
    w, h = 11, 6
    anims = []
    for d, b in PAIRS:  # the pair on frame 0 (PREVIOUS there acts as BACKGROUND), on a frame in the middle, and last
        anims.append(dict(w=w, h=h, frames=[frame(rng, fmt, 1, 1, 9, 4, d, b), frame(rng, fmt, 0, 0, w, h, NONE, OVER), frame(rng, fmt, 3, 2, 7, 4, d, b),
                                            frame(rng, fmt, 2, 0, 6, 6, NONE, OVER), frame(rng, fmt, 0, 3, 11, 3, d, b)]))
    # three PREVIOUS frames in a row over a canvas that stays, overlapping each other, then a frame that shows what is left
    anims.append(dict(w=w, h=h, frames=[frame(rng, fmt, 0, 0, w, h, NONE, SOURCE), frame(rng, fmt, 1, 1, 6, 4, PREVIOUS, OVER), frame(rng, fmt, 4, 0, 7, 5, PREVIOUS, SOURCE),
                                        frame(rng, fmt, 0, 2, 11, 4, PREVIOUS, OVER), frame(rng, fmt, 10, 5, 1, 1, NONE, OVER)]))
    got = check(engine, anims, fmt)
    # the restatement itself on the point of that animation: canvas 4 is canvas 0 but for its one pixel
    n = w * h * _px(fmt)
    c0, c4 = (np.frombuffer(got[-1][k * n:(k + 1) * n], dtype=_dtype(fmt)).reshape(h, w, 4) for k in (0, 4))
    assert (c0[:5] == c4[:5]).all() and (c0[5, :10] == c4[5, :10]).all()
    # PREVIOUS on frame 0 clears its region: frame 1 of that animation is drawn OVER transparent black everywhere, which copies
    # it (ba == 0) but for its own transparent pixels (fa == 0), which leave the black
    assert PAIRS[4] == (PREVIOUS, SOURCE)
    f1 = anims[4]["frames"][1]["px"]
    c1 = np.frombuffer(got[4][n:2 * n], dtype=_dtype(fmt)).reshape(h, w, 4)
    assert (c1 == np.where(f1[..., 3:4] == 0, 0, f1)).all()


def test_every_alpha_pair_at_rgba8(engine):
    """a 256x256 frame with fa = x over a canvas with ba = y: all 65536 (fa, ba) pairs, colours random"""
    rng = np.random.default_rng(8205)
    y, x = np.mgrid[0:256, 0:256]
    f0, f1 = frame(rng, RGBA8, 0, 0, 256, 256, NONE, SOURCE), frame(rng, RGBA8, 0, 0, 256, 256, NONE, OVER)
    f0["px"][..., 3], f1["px"][..., 3] = y, x
    got = check(engine, [dict(w=256, h=256, frames=[f0, f1])], RGBA8)[0]
    c1 = np.frombuffer(got[256 * 256 * 4:], dtype=np.uint8).reshape(256, 256, 4)
    # three pixels by hand: fa 0 keeps the canvas, fa 255 copies, and (fa, ba) = (100, 200) mixes
    assert (c1[200, 0] == f0["px"][200, 0]).all() and (c1[200, 255] == f1["px"][200, 255]).all()
    u, v = 100 * 255, 155 * 200
    f, b = f1["px"][200, 100].astype(int), f0["px"][200, 100].astype(int)
    assert list(c1[200, 100]) == [(f[k] * u + b[k] * v) // (u + v) for k in range(3)] + [(u + v) // 255]


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_a_batch_at_odd_output_alignments(engine, fmt):
    """animations of 1, 2 and 9 frames on canvases whose size is no multiple of 16, every output at another residue modulo 16:
    the alignment of a row differs from canvas to canvas, and wide and narrow stores alternate"""
    rng = np.random.default_rng(8207 + fmt)
    px = _px(fmt)
    anims = []
    for k, (w, h, n) in enumerate(((7, 3, 1), (9, 5, 2), (67, 3, 9), (13, 1, 9), (130, 2, 2), (4, 4, 9))):
        frames = []
        for j in range(n):
            fw, fh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
            frames.append(frame(rng, fmt, int(rng.integers(0, w - fw + 1)), int(rng.integers(0, h - fh + 1)), fw, fh, *PAIRS[(j + k) % 6]))
        anims.append(dict(w=w, h=h, frames=frames))
    residues = [(k * px) % 16 for k in range(1, len(anims) + 1)]
    assert len(set(residues)) == 16 // px
    check(engine, anims, fmt, residues=residues)


def test_a_stream_of_the_caller_and_an_empty_call(engine):
    import torch
    from zlibstream_amd import png_compose_batch_device
    rng = np.random.default_rng(8209)
    s = torch.cuda.Stream()
    anims = [dict(w=33, h=9, frames=[frame(rng, RGBA16, 0, 0, 33, 9, NONE, SOURCE), frame(rng, RGBA16, 5, 2, 20, 6, BACKGROUND, OVER),
                                     frame(rng, RGBA16, 0, 0, 33, 9, NONE, OVER)])]
    check(engine, anims, RGBA16, stream=s.cuda_stream)
    assert png_compose_batch_device(engine, [], [], [], [], []) is None


def test_the_stage_timer_shows_the_launch(engine):
    rng = np.random.default_rng(8210)
    engine.set_profiling(True)
    try:
        check(engine, [dict(w=40, h=8, frames=[frame(rng, RGBA8, 0, 0, 40, 8, NONE, SOURCE), frame(rng, RGBA8, 3, 1, 30, 5, PREVIOUS, OVER)])], RGBA8)
        ms = engine.stage_ms()
    finally:
        engine.set_profiling(False)
    assert ms.get("png_compose", 0) > 0, ms


def test_bad_arguments_are_stream_errors_and_touch_nothing(engine):
    import torch
    from zlibstream_amd import _native
    L = _native.lib()
    VP, I64, I32, FR = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, _native.PngFrame
    d_in = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    d_out = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pin, pout = d_in.data_ptr(), d_out.data_ptr()
    good = dict(x=1, y=1, width=2, height=2, dispose_op=0, blend_op=0)

    def call(n=1, ctx=engine.handle, px=((pin, pin),), frames=((good, good),), nf=(2,), w=(4,), h=(3,), fmt=RGBA8, out=(pout,), null_px_list=False,
             null_frames_list=False):
        arr = lambda t, v: None if v is None else (t * len(v))(*v)
        keep = []
        if px is None:
            ppx = None
        else:
            rows = [None if null_px_list else arr(VP, p) for p in px]
            keep += rows
            ppx = (ctypes.POINTER(VP) * len(rows))(*[ctypes.cast(r, ctypes.POINTER(VP)) if r is not None else ctypes.POINTER(VP)() for r in rows])
        if frames is None:
            pfr = None
        else:
            rows = [None if null_frames_list else (FR * len(fs))(*[FR(**f) for f in fs]) for fs in frames]
            keep += rows
            pfr = (ctypes.POINTER(FR) * len(rows))(*[ctypes.cast(r, ctypes.POINTER(FR)) if r is not None else ctypes.POINTER(FR)() for r in rows])
        return L.zs_png_compose_batch_device(ctx, n, ppx, pfr, arr(I32, nf), arr(I64, w), arr(I64, h), fmt, arr(VP, out), None)

    def fr(**kw):
        return ((dict(good, **kw), good),)

    bad = [dict(ctx=None), dict(n=-1), dict(px=None), dict(frames=None), dict(nf=None), dict(w=None), dict(h=None), dict(out=None),
           dict(null_px_list=True), dict(null_frames_list=True), dict(px=((pin, None),)), dict(out=(None,)),
           dict(nf=(0,)), dict(nf=(-1,)), dict(w=(0,)), dict(h=(0,)), dict(w=(1 << 31,)), dict(h=(1 << 31,)),
           dict(frames=fr(x=3)), dict(frames=fr(y=2)), dict(frames=fr(x=-1)), dict(frames=fr(y=-1)), dict(frames=fr(width=0)), dict(frames=fr(height=0)),
           dict(frames=fr(width=4)), dict(frames=fr(height=3)), dict(frames=fr(x=1 << 40)), dict(frames=fr(width=1 << 40)),
           dict(frames=fr(dispose_op=3)), dict(frames=fr(dispose_op=-1)), dict(frames=fr(blend_op=2)), dict(frames=fr(blend_op=-1)),
           dict(fmt=2), dict(fmt=-1), dict(out=(pout + 2,)), dict(px=((pin, pin + 1),)), dict(fmt=RGBA16, out=(pout + 4,)), dict(fmt=RGBA16, px=((pin + 4, pin),)),
           # more than 2^31 - 1 canvas rows in one call: refused before anything is read
           dict(n=2, px=((pin,), (pin,)), frames=((dict(good, x=0, width=1),), (dict(good, x=0, y=0, width=1, height=1),)), nf=(1, 1), w=(1, 1),
                h=((1 << 31) - 1, 1), out=(pout, pout))]
    for kw in bad:
        assert call(**kw) == ZS_STREAM_ERROR, kw
    assert call(n=0, px=None, frames=None, nf=None, w=None, h=None, out=None) == ZS_OK
    assert d_out.cpu().numpy().tobytes() == b"\xEE" * 4096
    # the same call with nothing wrong
    assert call() == ZS_OK
    got = d_out.cpu().numpy()
    assert (got[:96] == 0).all() and (got[96:] == 0xEE).all()  # (two canvases of 4 x 3 pixels: the frames hold zeros)
