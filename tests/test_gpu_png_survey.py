"""What an image's pixels allow (zs_png_survey_batch_device, KV), against a numpy survey written here from the struct's own
words in include/zsgpu.h: np.all for the flags, remainders for the sample depth, np.unique for the colours.  Every comparison is
exact, and a second run gives the same structs."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZS_OK, ZS_STREAM_ERROR = 0, -2
RGBA8, RGBA16 = 0, 1


def _top(fmt):
    return 65535 if fmt == RGBA16 else 255


def survey_ref(px, fmt):
    """(h, w, 4) int64 pixels -> the dict png_survey_batch_device returns"""
    r, g, b, a = (px[..., k] for k in range(4))
    low8 = fmt == RGBA8 or bool((px % 257 == 0).all())
    out = dict(opaque=int((a == _top(fmt)).all()), gray=int(((r == g) & (g == b)).all()), low8=int(low8), sample_depth=16, n_colors=257, colors=[])
    if not low8:
        return out
    p8 = px if fmt == RGBA8 else px // 257
    out["sample_depth"] = next(d for d in (1, 2, 4, 8) if (p8[..., :3] % (255 // ((1 << d) - 1)) == 0).all())
    colors = np.unique(p8.reshape(-1, 4), axis=0)
    if len(colors) <= 256:
        order = np.lexsort((colors[:, 2], colors[:, 1], colors[:, 0], colors[:, 3]))  # by A, then R, G, B
        out["n_colors"], out["colors"] = len(colors), [tuple(int(v) for v in c) for c in colors[order]]
    return out


def _cuda(px, fmt):
    import torch
    return torch.from_numpy(np.frombuffer(px.astype("<u2" if fmt == RGBA16 else np.uint8).tobytes(), dtype=np.uint8).copy()).cuda()


def run_survey(engine, pxs, fmt, stream=None):
    import torch
    from zlibstream_amd import png_survey_batch_device
    d_in = [_cuda(p, fmt) for p in pxs]
    torch.cuda.synchronize()
    return png_survey_batch_device(engine, [t.data_ptr() for t in d_in], [p.shape[1] for p in pxs], [p.shape[0] for p in pxs], format=fmt, stream=stream)


def check(engine, pxs, fmt):
    got = run_survey(engine, pxs, fmt)
    want = [survey_ref(p, fmt) for p in pxs]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, pxs[k].shape, {f: (g[f], w[f]) for f in ("opaque", "gray", "low8", "sample_depth", "n_colors")})
    return got


def plain(w, h, fmt, value=255):
    """opaque, gray, one colour"""
    m = 257 if fmt == RGBA16 else 1
    px = np.full((h, w, 4), value * m, dtype=np.int64)
    px[..., 3] = _top(fmt)
    return px


SHAPES = ((1, 1), (7, 300), (1000, 3))
ENDS = ("first", "last")


def _at(px, end):
    return (0, 0) if end == "first" else (px.shape[0] - 1, px.shape[1] - 1)


# ---------------------------------------------------------------- the flags
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_one_pixel_breaks_a_flag_at_either_end(engine, fmt):
    """an image that is opaque, gray, of one sample bit and one colour; then one pixel -- the first, or the last of the last row
    -- with another alpha, another G, (RGBA16) another low byte in one sample"""
    pxs, broken = [], []
    for w, h in SHAPES:
        base = plain(w, h, fmt)
        pxs.append(base), broken.append(None)
        for end in ENDS:
            y, x = _at(base, end)
            for flag in ("opaque", "gray") + (("low8",) if fmt == RGBA16 else ()):
                p = base.copy()
                if flag == "opaque":
                    p[y, x, 3] = _top(fmt) - (257 if fmt == RGBA16 else 1)
                elif flag == "gray":
                    p[y, x, 1] = 0
                else:
                    p[y, x, 2] -= 1  # 0xFFFE: the low byte alone
                pxs.append(p), broken.append(flag)
    got = check(engine, pxs, fmt)
    for g, flag in zip(got, broken):
        flags = {f: g[f] for f in ("opaque", "gray", "low8")}
        assert flags == {f: int(f != flag and not (flag == "low8" and f == "gray")) for f in flags}, (flag, flags)
        if flag is None:
            assert (g["sample_depth"], g["n_colors"], g["colors"]) == (1, 1, [(255, 255, 255, 255)])


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_sample_depth_takes_each_of_its_values(engine, fmt):
    """samples that are multiples of 255, of 85, of 17, any -- broken by one sample at either end -- and, at RGBA16, samples
    that are no multiples of 257.  The alpha samples do not count."""
    rng = np.random.default_rng(9601 + fmt)
    m = 257 if fmt == RGBA16 else 1
    pxs, depths = [], []
    for w, h in SHAPES:
        for d, step in ((1, 255), (2, 85), (4, 17), (8, 1)):
            p = rng.integers(0, 255 // step + 1, (h, w, 4)).astype(np.int64) * step * m
            p[..., 3] = rng.integers(0, 256, (h, w)) * m
            y, x = _at(p, ENDS[d % 2])
            p[y, x, d % 3] = {1: 255, 2: 85, 4: 17, 8: 3}[d] * m  # at least one pixel needs that depth
            pxs.append(p), depths.append(d)
        if fmt == RGBA16:
            p = plain(w, h, fmt)
            y, x = _at(p, "last")
            p[y, x, 0] = 0x1234
            pxs.append(p), depths.append(16)
    got = check(engine, pxs, fmt)
    assert [g["sample_depth"] for g in got] == depths
    assert set(depths) == ({1, 2, 4, 8, 16} if fmt == RGBA16 else {1, 2, 4, 8})


# ---------------------------------------------------------------- the colours
def _colors(n, seed):
    """n different RGBA8 colours, (n, 4)"""
    c = np.random.default_rng(seed).choice(1 << 32, size=n, replace=False).astype(np.uint64)
    return np.stack([(c >> s) & 255 for s in (0, 8, 16, 24)], axis=1).astype(np.int64)


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_colour_counts(engine, fmt):
    m = 257 if fmt == RGBA16 else 1
    rng = np.random.default_rng(9602 + fmt)
    pxs = []
    # exactly 256 and 257 colours, scattered over 40 x 40
    for n in (256, 257):
        c = _colors(n, 9610 + n)
        idx = np.concatenate([np.arange(n), rng.integers(0, n, 1600 - n)])
        pxs.append(c[rng.permutation(idx)].reshape(40, 40, 4) * m)
    # two colours that differ in alpha alone
    p = plain(33, 31, fmt, 90)
    p[17, 5, 3] = 254 * m
    pxs.append(p)
    # 0x00000000 and 0xFFFFFFFF both present, and alone
    p = plain(7, 300, fmt)
    p[::2] = 0
    pxs.append(p)
    pxs.append(plain(1, 1, fmt) * 0)
    # 256 colours and white for the 257th: no workgroup's table holds more than 256
    c = _colors(256, 9620)
    c[c.sum(axis=1) == 4 * 255] = 1
    p = np.concatenate([c, np.full((144, 4), 255, dtype=np.int64)]).reshape(20, 20, 4) * m
    pxs.append(p)
    # 257 colours, one to a row of 16 pixels over 257 rows: a workgroup of any run of fewer than 257 rows sees fewer than 257,
    # the merge must find the overflow; and 256 the same way, which it must not
    for n in (257, 256):
        pxs.append(np.repeat(_colors(n, 9630 + n)[:, None, :], 16, axis=1) * m)
    # 200 colours, all of them in every row of 64 rows: every workgroup meets them all
    pxs.append(np.repeat(_colors(200, 9640)[None, :, :], 64, axis=0)[:, rng.permutation(200)] * m)
    got = check(engine, pxs, fmt)
    assert [g["n_colors"] for g in got] == [256, 257, 2, 2, 1, 257, 257, 256, 200]
    assert got[2]["colors"] == [(90, 90, 90, 254), (90, 90, 90, 255)] and got[3]["colors"] == [(0, 0, 0, 0), (255, 255, 255, 255)] and got[4]["colors"] == [(0, 0, 0, 0)]
    assert got[1]["colors"] == [] and len(got[0]["colors"]) == 256


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16])
def test_a_mixed_batch_equals_the_single_calls_and_a_second_run(engine, fmt):
    rng = np.random.default_rng(9603 + fmt)
    m = 257 if fmt == RGBA16 else 1
    pxs = []
    for k, (w, h) in enumerate(SHAPES + ((33, 31), (257, 5), (640, 97))):
        p = rng.integers(0, 1 << (1 + k), (h, w, 4)).astype(np.int64) * (255 // ((1 << (1 + k)) - 1) if k < 3 else 1) * m
        if k % 2:
            p[..., 3] = _top(fmt)
        if k == 4:
            p[..., 1] = p[..., 2] = p[..., 0]
        pxs.append(p)
    if fmt == RGBA16:
        pxs.append(rng.integers(0, 65536, (9, 130, 4)).astype(np.int64))  # low8 false
        pxs.append(rng.integers(0, 256, (9, 130, 4)).astype(np.int64) * 257)  # low8 true
    got = check(engine, pxs, fmt)
    assert run_survey(engine, pxs, fmt) == got
    for p, g in zip(pxs, got):
        assert run_survey(engine, [p], fmt) == [g]
    if fmt == RGBA16:
        assert (got[-2]["low8"], got[-2]["sample_depth"], got[-2]["n_colors"]) == (0, 16, 257) and got[-1]["low8"] == 1


# ---------------------------------------------------------------- the rest
def test_a_stream_of_the_caller_an_empty_call_and_the_stage_timer(engine):
    import torch
    from zlibstream_amd import png_survey_batch_device
    rng = np.random.default_rng(9604)
    pxs = [rng.integers(0, 4, (31, 33, 4)).astype(np.int64) * 85, plain(1000, 3, RGBA8)]
    s = torch.cuda.Stream()
    assert run_survey(engine, pxs, RGBA8, stream=s.cuda_stream) == [survey_ref(p, RGBA8) for p in pxs]
    assert png_survey_batch_device(engine, [], [], []) == []
    engine.set_profiling(True)
    try:
        got = run_survey(engine, pxs, RGBA8)
        stages = engine.stage_ms()
    finally:
        engine.set_profiling(False)
    assert got == [survey_ref(p, RGBA8) for p in pxs] and stages.get("png_survey", 0) > 0, stages


def test_bad_arguments_are_stream_errors_and_touch_nothing(engine):
    from zlibstream_amd import _native
    L = _native.lib()
    d_in = _cuda(plain(3, 4, RGBA16), RGBA16)
    VP, I64 = ctypes.c_void_p, ctypes.c_int64
    out = (_native.PngSurvey * 2)()
    ctypes.memset(out, 0x5A, ctypes.sizeof(out))
    before = bytes(out)

    def call(n=1, ctx=engine.handle, inp=(d_in.data_ptr(),), w=(3,), h=(4,), fmt=RGBA8, res=out):
        arr = lambda t, v: None if v is None else (t * len(v))(*v)
        return L.zs_png_survey_batch_device(ctx, n, arr(VP, inp), arr(I64, w), arr(I64, h), fmt, res, None)

    for kw in (dict(ctx=None), dict(n=-1), dict(inp=None), dict(w=None), dict(h=None), dict(res=None), dict(inp=(None,)), dict(w=(0,)), dict(w=(1 << 31,)),
               dict(h=(0,)), dict(h=(1 << 31,)), dict(w=(-1,)), dict(fmt=2), dict(fmt=-1), dict(inp=(d_in.data_ptr() + 2,)), dict(inp=(d_in.data_ptr() + 1,)),
               dict(fmt=RGBA16, inp=(d_in.data_ptr() + 4,))):
        assert call(**kw) == ZS_STREAM_ERROR, kw
    assert call(n=0, inp=None, w=None, h=None, res=None) == ZS_OK
    assert bytes(out) == before
    assert call(fmt=RGBA16) == ZS_OK
    assert (out[0].opaque, out[0].gray, out[0].low8, out[0].sample_depth, out[0].n_colors, tuple(out[0].colors[0]), tuple(out[0].colors[1])) == \
        (1, 1, 1, 1, 1, (255, 255, 255, 255), (0, 0, 0, 0))
    assert bytes(out)[ctypes.sizeof(_native.PngSurvey):] == before[ctypes.sizeof(_native.PngSurvey):]
