"""Python mirror of the reference's Stream-level API for the deflate path.

Names, argument meaning and error behaviour follow src/ZlibStream/
ZlibOutputStream.cs, ZlibOptions.cs, CompressionLevel.cs,
CompressionStrategy.cs, FlushMode.cs, ZlibStreamException.cs and
ThrowHelper.cs:21-23 of the reference, so that the parity tests read like the
reference's own (tests/ZlibStream.Tests/ZlibStreamTests.Roundtrip.cs).
"""
import ctypes
import enum
import io

from . import _native


class CompressionLevel(enum.IntEnum):  # CompressionLevel.cs
    DefaultCompression = -1
    Level0 = 0
    NoCompression = 0
    Level1 = 1
    BestSpeed = 1
    Level2 = 2
    Level3 = 3
    Level4 = 4
    Level5 = 5
    Level6 = 6
    Level7 = 7
    Level8 = 8
    Level9 = 9
    BestCompression = 9


class CompressionStrategy(enum.IntEnum):  # CompressionStrategy.cs
    DefaultStrategy = 0
    Filtered = 1
    HuffmanOnly = 2
    Rle = 3
    Fixed = 4


class FlushMode(enum.IntEnum):  # FlushMode.cs
    NoFlush = 0
    PartialFlush = 1
    SyncFlush = 2
    FullFlush = 3
    Finish = 4


class CompressionState(enum.IntEnum):  # CompressionState.cs
    ZVERSIONERROR = -6
    ZBUFERROR = -5
    ZMEMERROR = -4
    ZDATAERROR = -3
    ZSTREAMERROR = -2
    ZERRNO = -1
    ZOK = 0
    ZSTREAMEND = 1
    ZNEEDDICT = 2


class ZlibStreamException(Exception):  # ZlibStreamException.cs
    pass


class ZlibOptions:  # ZlibOptions.cs
    def __init__(self, CompressionLevel=None, CompressionStrategy=CompressionStrategy.DefaultStrategy,
                 FlushMode=FlushMode.NoFlush):
        self.CompressionLevel = CompressionLevel
        self.CompressionStrategy = CompressionStrategy
        self.FlushMode = FlushMode


def deflate_bound(n):
    return int(_native.lib().zs_deflate_bound(int(n)))


class Engine:
    """One zs_ctx: a GPU plus its reusable workspace."""

    def __init__(self, device=0):
        self._lib = _native.lib()
        h = ctypes.c_void_p()
        rc = self._lib.zs_ctx_create(int(device), ctypes.byref(h))
        if rc != 0 or not h:
            raise RuntimeError("zs_ctx_create(device=%d) failed with %d: no usable MI355X / HIP device. "
                               "There is no CPU fallback." % (device, rc))
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.zs_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def last_error(self):
        return (self._lib.zs_ctx_last_error(self._h) or b"").decode()

    def set_profiling(self, on):
        self._lib.zs_ctx_set_profiling(self._h, 1 if on else 0)

    def counter(self, name):
        """zs_ctx_counter: "fast_rounds", "fast_fallbacks", "round_runs", "cut_rounds", "lit_fallbacks", "lit_engine_bytes",
        "spec_streams", "spec_fallbacks", "spec_periodic", "spec_wrong_chunks", "png_segments", "inf_lane_streams" (streams of
        the last inflate call whose chain had blocks for the lane decoder: checkpoints and no tokens), "inf_wave_streams"
        (streams of the last inflate call at or above the block-parallel minimum that the block-parallel pass handed to the
        one-wave decoder; streams below the minimum are not counted), "plan_reused" (1: the last deflate call had the shape
        of the one before and took its plan)."""
        return int(self._lib.zs_ctx_counter(self._h, name.encode()))

    def stage_ms(self):
        n = self._lib.zs_ctx_stage_count(self._h)
        return {self._lib.zs_ctx_stage_name(self._h, i).decode(): self._lib.zs_ctx_stage_ms(self._h, i) for i in range(n)}

    def _call_batch(self, fn, in_ptrs, in_lens, out_ptrs, out_caps, level, strategy, hash_variant, extra=()):
        n = len(in_ptrs)
        VP = ctypes.c_void_p * n
        I64 = ctypes.c_int64 * n
        I32 = ctypes.c_int * n
        out_len = I64()
        status = I32()
        rc = fn(self._h, n, VP(*in_ptrs), I64(*in_lens), VP(*out_ptrs), I64(*out_caps), out_len, status, int(level),
                int(strategy), int(hash_variant), *extra)
        return rc, list(out_len), list(status)

    class DeviceBatch:
        """The four argument arrays of zs_deflate_batch_device as C arrays, made once: a C# or C++ caller hands the library
        arrays it already has, while turning Python lists of thousands of streams into ctypes arrays costs a millisecond or
        two per call -- as much as the device takes for a tenth of such a batch."""

        def __init__(self, in_ptrs, in_lens, out_ptrs, out_caps):
            n = self.n = len(in_ptrs)
            self.in_ptrs = (ctypes.c_void_p * n)(*in_ptrs)
            self.in_lens = (ctypes.c_int64 * n)(*in_lens)
            self.out_ptrs = (ctypes.c_void_p * n)(*out_ptrs)
            self.out_caps = (ctypes.c_int64 * n)(*out_caps)
            self.out_len = (ctypes.c_int64 * n)()
            self.status = (ctypes.c_int * n)()

    def deflate_device_batch(self, batch, level=6, strategy=0, hash_variant=0, stream=None):
        """zs_deflate_batch_device on a DeviceBatch; the output lengths are left in batch.out_len (a C array)."""
        rc = self._lib.zs_deflate_batch_device(self._h, batch.n, batch.in_ptrs, batch.in_lens, batch.out_ptrs, batch.out_caps,
                                               batch.out_len, batch.status, int(level), int(strategy), int(hash_variant),
                                               ctypes.c_void_p(stream or 0))
        if rc != 0:
            raise ZlibStreamException("deflating: " + self.last_error())
        return batch.out_len

    def deflate_batch_device(self, in_ptrs, in_lens, out_ptrs, out_caps, level=6, strategy=0, hash_variant=0, stream=None):
        """Device-resident buffers (raw device pointers as ints).  Returns the output lengths."""
        rc, lens, status = self._call_batch(self._lib.zs_deflate_batch_device, in_ptrs, in_lens, out_ptrs, out_caps, level,
                                            strategy, hash_variant, (ctypes.c_void_p(stream or 0),))
        if rc != 0:
            raise ZlibStreamException("deflating: " + self.last_error())
        return lens

    def deflate_writes_device(self, in_ptr, in_len, write_ends, out_ptr, out_cap, level=6, strategy=0, hash_variant=0, stream=None):
        """One device-resident stream written in several NoFlush Writes (zs_deflate_writes_device): `write_ends` are the
        cumulative Write ends (a sequence of ints or a ctypes int64 array).  Returns the output length."""
        if not isinstance(write_ends, ctypes.Array):
            write_ends = (ctypes.c_int64 * len(write_ends))(*write_ends)
        olen = ctypes.c_int64(0)
        rc = self._lib.zs_deflate_writes_device(self._h, ctypes.c_void_p(in_ptr), int(in_len), write_ends, len(write_ends),
                                                ctypes.c_void_p(out_ptr), int(out_cap), ctypes.byref(olen), int(level), int(strategy),
                                                int(hash_variant), ctypes.c_void_p(stream or 0))
        if rc != 0:
            raise ZlibStreamException("deflating: " + self.last_error())
        return olen.value

    def deflate_writes_batch_device(self, in_ptrs, in_lens, write_ends, out_ptrs, out_caps, level=6, strategy=0, hash_variant=0, stream=None,
                                    return_status=False):
        """n device-resident streams, each written in its own NoFlush Writes (zs_deflate_writes_batch_device).  write_ends: None
        (every stream one Write: deflate_batch_device), or per stream None (one Write) or its cumulative Write ends -- a
        sequence of ints or a ctypes int64 array, non-decreasing, the last one = in_lens[i].  Returns the output lengths; with
        return_status=True nothing is raised for a failing stream and (code, lengths, per-stream codes) comes back (-5,
        ZS_BUF_ERROR, for a stream whose capacity was too small; the other streams are complete).  A stream takes the path it
        takes alone through deflate_writes_device: scanline Writes at levels 1-3 often mean the one-wave literal engine."""
        n = len(in_ptrs)
        if not (len(in_lens) == len(out_ptrs) == len(out_caps) == n) or (write_ends is not None and len(write_ends) != n):
            raise ValueError("deflate_writes_batch_device: the argument lists differ in length")
        arrays = []
        for i in range(n):
            we = write_ends[i] if write_ends is not None else None
            if we is None:
                arrays.append(None)
                continue
            prev = 0
            for e in we:
                if int(e) < prev:
                    raise ValueError("deflate_writes_batch_device: the Write ends of stream %d decrease" % i)
                prev = int(e)
            if len(we) and prev != int(in_lens[i]):
                raise ValueError("deflate_writes_batch_device: the last Write end of stream %d is not its length" % i)
            arrays.append(we if isinstance(we, ctypes.Array) else (ctypes.c_int64 * len(we))(*[int(e) for e in we]))
        if n == 0:
            return (0, [], []) if return_status else []
        P64 = ctypes.POINTER(ctypes.c_int64)
        ends = None
        if write_ends is not None:
            ends = (P64 * n)(*[ctypes.cast(a, P64) if a is not None and len(a) else P64() for a in arrays])
        counts = (ctypes.c_int64 * n)(*[len(a) if a is not None else 0 for a in arrays])
        VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
        out_len, status = I64(), I32()
        rc = self._lib.zs_deflate_writes_batch_device(self._h, n, VP(*[int(p) for p in in_ptrs]), I64(*[int(x) for x in in_lens]), ends, counts,
                                                      VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), out_len, status,
                                                      int(level), int(strategy), int(hash_variant), ctypes.c_void_p(stream or 0))
        if return_status:
            return rc, list(out_len), list(status)
        if rc != 0:
            raise ZlibStreamException("deflating: " + self.last_error())
        return list(out_len)

    def deflate_batch(self, buffers, level=6, strategy=0, hash_variant=0):
        """Host buffers (bytes-like) -> list of zlib streams (bytes)."""
        bufs = [bytes(b) for b in buffers]
        n = len(bufs)
        if n == 0:
            return []
        keep = [ctypes.create_string_buffer(b, len(b)) if len(b) else ctypes.create_string_buffer(1) for b in bufs]
        caps = [deflate_bound(len(b)) for b in bufs]
        outs = [ctypes.create_string_buffer(c) for c in caps]
        rc, lens, status = self._call_batch(self._lib.zs_deflate_batch, [ctypes.addressof(k) for k in keep],
                                            [len(b) for b in bufs], [ctypes.addressof(o) for o in outs], caps, level,
                                            strategy, hash_variant)
        if rc != 0:
            raise ZlibStreamException("deflating: " + self.last_error())
        return [outs[i].raw[:lens[i]] for i in range(n)]


    def _call_inflate(self, fn, in_ptrs, in_lens, out_ptrs, out_caps, extra=()):
        n = len(in_ptrs)
        VP = ctypes.c_void_p * n
        I64 = ctypes.c_int64 * n
        I32 = ctypes.c_int * n
        out_len = I64()
        status = I32()
        rc = fn(self._h, n, VP(*in_ptrs), I64(*in_lens), VP(*out_ptrs), I64(*out_caps), out_len, status, *extra)
        return rc, list(out_len), list(status)

    def inflate_batch_device(self, in_ptrs, in_lens, out_ptrs, out_caps, stream=None):
        rc, lens, status = self._call_inflate(self._lib.zs_inflate_batch_device, in_ptrs, in_lens, out_ptrs, out_caps,
                                              (ctypes.c_void_p(stream or 0),))
        if rc != 0:
            raise ZlibStreamException("inflating: " + self.last_error())  # ThrowHelper.cs:21-23
        return lens

    def inflate_batch(self, streams, out_sizes):
        """Host buffers: zlib streams -> decoded bytes; out_sizes[i] is the capacity for stream i."""
        zs = [bytes(z) for z in streams]
        n = len(zs)
        if n == 0:
            return []
        keep = [ctypes.create_string_buffer(z, len(z)) if len(z) else ctypes.create_string_buffer(1) for z in zs]
        outs = [ctypes.create_string_buffer(max(int(c), 1)) for c in out_sizes]
        rc, lens, status = self._call_inflate(self._lib.zs_inflate_batch, [ctypes.addressof(k) for k in keep], [len(z) for z in zs],
                                              [ctypes.addressof(o) for o in outs], [int(c) for c in out_sizes])
        if rc != 0:
            raise ZlibStreamException("inflating: " + self.last_error())
        return [outs[i].raw[:lens[i]] for i in range(n)]


def deflate_batch_multi(engines, buffers, level=6, strategy=0, hash_variant=0):
    """Host buffers sharded over several engines (one per GPU) by zs_deflate_batch_multi -> zlib streams in input order."""
    lib = _native.lib()
    bufs = [bytes(b) for b in buffers]
    n = len(bufs)
    if n == 0:
        return []
    keep = [ctypes.create_string_buffer(b, len(b)) if len(b) else ctypes.create_string_buffer(1) for b in bufs]
    caps = [deflate_bound(len(b)) for b in bufs]
    outs = [ctypes.create_string_buffer(c) for c in caps]
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status = I64(), I32()
    ctxs = (ctypes.c_void_p * len(engines))(*[e.handle for e in engines])
    rc = lib.zs_deflate_batch_multi(ctxs, len(engines), n, VP(*[ctypes.addressof(k) for k in keep]), I64(*[len(b) for b in bufs]),
                                    VP(*[ctypes.addressof(o) for o in outs]), I64(*caps), out_len, status, int(level), int(strategy),
                                    int(hash_variant))
    if rc != 0:
        bad = [e.last_error() for e in engines if e.last_error()]
        raise ZlibStreamException("deflating: " + (bad[0] if bad else "error %d" % rc))
    return [outs[i].raw[:out_len[i]] for i in range(n)]


def inflate_batch_multi(engines, streams, out_sizes):
    """zlib streams sharded over several engines by zs_inflate_batch_multi -> decoded bytes in input order."""
    lib = _native.lib()
    zs = [bytes(z) for z in streams]
    n = len(zs)
    if n == 0:
        return []
    keep = [ctypes.create_string_buffer(z, len(z)) if len(z) else ctypes.create_string_buffer(1) for z in zs]
    outs = [ctypes.create_string_buffer(max(int(c), 1)) for c in out_sizes]
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status = I64(), I32()
    ctxs = (ctypes.c_void_p * len(engines))(*[e.handle for e in engines])
    rc = lib.zs_inflate_batch_multi(ctxs, len(engines), n, VP(*[ctypes.addressof(k) for k in keep]), I64(*[len(z) for z in zs]),
                                    VP(*[ctypes.addressof(o) for o in outs]), I64(*[int(c) for c in out_sizes]), out_len, status)
    if rc != 0:
        bad = [e.last_error() for e in engines if e.last_error()]
        raise ZlibStreamException("inflating: " + (bad[0] if bad else "error %d" % rc))
    return [outs[i].raw[:out_len[i]] for i in range(n)]


def _multi_device_call(fn_name, engines, in_ptrs, in_lens, out_ptrs, out_caps, part_of, extra=()):
    lib = _native.lib()
    n = len(in_ptrs)
    VP, I64, I32 = ctypes.c_void_p * max(n, 1), ctypes.c_int64 * max(n, 1), ctypes.c_int * max(n, 1)
    out_len, status = I64(), I32()
    ctxs = (ctypes.c_void_p * len(engines))(*[e.handle for e in engines])
    rc = getattr(lib, fn_name)(ctxs, len(engines), n, VP(*[int(p) for p in in_ptrs]), I64(*[int(x) for x in in_lens]), VP(*[int(p) for p in out_ptrs]),
                               I64(*[int(x) for x in out_caps]), out_len, status, I32(*[int(x) for x in part_of]), *extra)
    return rc, list(out_len)[:n], list(status)[:n]


def deflate_batch_multi_device(engines, in_ptrs, in_lens, out_ptrs, out_caps, part_of, level=6, strategy=0, hash_variant=0):
    """Device-resident buffers sharded over several engines (zs_deflate_batch_multi_device): buffer i and its output live on
    the GPU of engines[part_of[i]] (shard.partition / zs_partition gives a balanced part_of).  -> compressed lengths."""
    rc, lens, _ = _multi_device_call("zs_deflate_batch_multi_device", engines, in_ptrs, in_lens, out_ptrs, out_caps, part_of,
                                     (int(level), int(strategy), int(hash_variant)))
    if rc != 0:
        bad = [e.last_error() for e in engines if e.last_error()]
        raise ZlibStreamException("deflating: " + (bad[0] if bad else "error %d" % rc))
    return lens


def inflate_batch_multi_device(engines, in_ptrs, in_lens, out_ptrs, out_caps, part_of):
    """Device-resident zlib streams sharded over several engines (zs_inflate_batch_multi_device).  -> decoded lengths."""
    rc, lens, _ = _multi_device_call("zs_inflate_batch_multi_device", engines, in_ptrs, in_lens, out_ptrs, out_caps, part_of)
    if rc != 0:
        bad = [e.last_error() for e in engines if e.last_error()]
        raise ZlibStreamException("inflating: " + (bad[0] if bad else "error %d" % rc))
    return lens


def device_count():
    return int(_native.lib().zs_device_count())


def png_filter_device(engine, pixels_ptr, row_bytes, height, bpp, filter_type, out_ptr, stream=None):
    """PNG scanline filtering of a device-resident image into a device buffer of height * (row_bytes + 1) bytes."""
    rc = _native.lib().zs_png_filter_device(engine.handle, ctypes.c_void_p(pixels_ptr), int(row_bytes), int(height), int(bpp),
                                            int(filter_type), ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0))
    if rc != 0:
        raise ValueError("zs_png_filter_device rejected the arguments (%d)" % rc)


def _png_filter_check(name, ptrs, row_bytes, heights, bpps, filters, out_ptrs):
    n = len(ptrs)
    if not (len(row_bytes) == len(heights) == len(bpps) == len(filters) == len(out_ptrs) == n):
        raise ValueError(name + ": the argument lists differ in length")
    for p, rb, h, b, f, o in zip(ptrs, row_bytes, heights, bpps, filters, out_ptrs):
        if not p or not o or int(rb) < 1 or not 1 <= int(h) <= 0x7FFFFFFF or not 1 <= int(b) <= 8 or not 0 <= int(f) <= 5:
            raise ValueError(name + ": row_bytes >= 1, 1 <= height <= 2^31 - 1, bpp 1..8, filter 0..5 and non-null device pointers are required")
    if sum(int(h) for h in heights) > 0x7FFFFFFF:
        raise ValueError(name + ": more than 2^31 - 1 rows in one call")
    return n


def png_filter_batch_device(engine, pixel_ptrs, row_bytes, heights, bpps, filters, out_ptrs, stream=None):
    """png_filter_device for many device-resident images in one launch: image i's height * (row_bytes + 1) filtered bytes
    go to out_ptrs[i], byte for byte what the single call writes (filters[i] 0..5, 5 = adaptive)."""
    n = _png_filter_check("png_filter_batch_device", pixel_ptrs, row_bytes, heights, bpps, filters, out_ptrs)
    if n == 0:
        return
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    rc = _native.lib().zs_png_filter_batch_device(engine.handle, n, VP(*[int(p) for p in pixel_ptrs]), I64(*[int(x) for x in row_bytes]),
                                                  I64(*[int(x) for x in heights]), I32(*[int(x) for x in bpps]), I32(*[int(x) for x in filters]),
                                                  VP(*[int(p) for p in out_ptrs]), ctypes.c_void_p(stream or 0))
    if rc != 0:
        raise ValueError("zs_png_filter_batch_device failed (%d): %s" % (rc, engine.last_error()))


def png_idat_batch_device(engine, pixel_ptrs, row_bytes, heights, bpps, filters, out_ptrs, out_caps, rows_per_write=1, level=6, strategy=0,
                          hash_variant=0, stream=None, return_status=False):
    """Pixels -> IDAT payloads for many device-resident images in one call (zs_png_idat_batch_device): the batch filter into
    a buffer the engine keeps, then every image's rows as the Writes of its own zlib stream -- rows_per_write rows a Write
    (1: the scanline-by-scanline encoder; 0: one Write per image).  Returns the stream lengths; return_status as
    Engine.deflate_writes_batch_device.  At levels 1-3 scanline Writes often put a stream on the one-wave literal engine,
    as they do one image at a time."""
    if len(out_caps) != len(pixel_ptrs):
        raise ValueError("png_idat_batch_device: the argument lists differ in length")
    n = _png_filter_check("png_idat_batch_device", pixel_ptrs, row_bytes, heights, bpps, filters, out_ptrs)
    if int(rows_per_write) < 0:
        raise ValueError("png_idat_batch_device: rows_per_write is negative")
    if n == 0:
        return (0, [], []) if return_status else []
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status = I64(), I32()
    rc = _native.lib().zs_png_idat_batch_device(engine.handle, n, VP(*[int(p) for p in pixel_ptrs]), I64(*[int(x) for x in row_bytes]),
                                                I64(*[int(x) for x in heights]), I32(*[int(x) for x in bpps]), I32(*[int(x) for x in filters]),
                                                int(rows_per_write), VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), out_len,
                                                status, int(level), int(strategy), int(hash_variant), ctypes.c_void_p(stream or 0))
    if return_status:
        return rc, list(out_len), list(status)
    if rc != 0:
        raise ZlibStreamException("deflating: " + engine.last_error())
    return list(out_len)


def _png_unfilter_check(in_ptr, row_bytes, height, bpp, out_ptr):
    if not in_ptr or not out_ptr or int(row_bytes) < 1 or not 1 <= int(height) <= 0x7FFFFFFF or not 1 <= int(bpp) <= 8:
        raise ValueError("png_unfilter: row_bytes >= 1, 1 <= height <= 2^31 - 1, bpp 1..8 and non-null device pointers are required")


def png_unfilter_device(engine, in_ptr, row_bytes, height, bpp, out_ptr, stream=None):
    """PNG scanline reconstruction (the inverse of png_filter_device) of a device-resident filtered image -- height rows of
    1 + row_bytes bytes, what inflate_batch_device leaves for an IDAT payload -- into height * row_bytes bytes of pixels in
    a device buffer.  Returns when the pixels are written.  A filter-type byte above 4 raises ZlibStreamException."""
    _png_unfilter_check(in_ptr, row_bytes, height, bpp, out_ptr)
    rc = _native.lib().zs_png_unfilter_device(engine.handle, ctypes.c_void_p(in_ptr), int(row_bytes), int(height), int(bpp),
                                              ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0))
    if rc == -3:
        raise ZlibStreamException("png: " + engine.last_error())
    if rc != 0:
        raise ValueError("zs_png_unfilter_device failed (%d): %s" % (rc, engine.last_error()))


def png_unfilter_batch_device(engine, in_ptrs, row_bytes, heights, bpps, out_ptrs, stream=None):
    """Many independent filtered images (the images of a batch, the Adam7 passes of one) in one call -> a status per image:
    0, or -3 (ZS_DATA_ERROR) for an image with a filter-type byte above 4 (engine.last_error() names the first such image
    and row; the other images are reconstructed all the same)."""
    n = len(in_ptrs)
    if not (len(row_bytes) == len(heights) == len(bpps) == len(out_ptrs) == n):
        raise ValueError("png_unfilter_batch_device: the argument lists differ in length")
    if n == 0:
        return []
    for a in zip(in_ptrs, row_bytes, heights, bpps, out_ptrs):
        _png_unfilter_check(*a)
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    status = I32()
    rc = _native.lib().zs_png_unfilter_batch_device(engine.handle, n, VP(*[int(p) for p in in_ptrs]), I64(*[int(x) for x in row_bytes]),
                                                    I64(*[int(x) for x in heights]), I32(*[int(x) for x in bpps]),
                                                    VP(*[int(p) for p in out_ptrs]), status, ctypes.c_void_p(stream or 0))
    if rc not in (0, -3):
        raise ValueError("zs_png_unfilter_batch_device failed (%d): %s" % (rc, engine.last_error()))
    return list(status)


PNG_BITS_PER_PIXEL = (1, 2, 4, 8, 16, 24, 32, 48, 64)


def png_idat_layout(width, height, bits_per_pixel, interlace):
    """zs_png_idat_layout (host code, no GPU): (inflated size of the IDAT payload, row_bytes[7], rows[7]) -- for an interlaced
    image the seven Adam7 passes, 0 / 0 for an absent one; otherwise entry 0 is the image.  ValueError for bad arguments."""
    rb, rows = (ctypes.c_int64 * 7)(), (ctypes.c_int64 * 7)()
    width, height, bits_per_pixel, interlace = int(width), int(height), int(bits_per_pixel), int(interlace)
    ok = 1 <= width <= 0x7FFFFFFF and 1 <= height <= 0x7FFFFFFF and bits_per_pixel in PNG_BITS_PER_PIXEL and interlace in (0, 1)
    total = _native.lib().zs_png_idat_layout(width, height, bits_per_pixel, interlace, rb, rows) if ok else -1
    if total < 0:
        raise ValueError("png_idat_layout: 1 <= width, height <= 2^31 - 1, bits_per_pixel in %r and interlace 0 or 1 are required" % (PNG_BITS_PER_PIXEL,))
    return int(total), list(rb), list(rows)


def _png_image_check(name, ptrs, widths, heights, bits, interlace, out_ptrs):
    """-> the rows the call works on, pass rows counted"""
    n = len(ptrs)
    if not (len(widths) == len(heights) == len(bits) == len(interlace) == len(out_ptrs) == n):
        raise ValueError(name + ": the argument lists differ in length")
    total_rows = 0
    for p, w, h, b, il, o in zip(ptrs, widths, heights, bits, interlace, out_ptrs):
        if not p or not o or not 1 <= int(w) <= 0x7FFFFFFF or not 1 <= int(h) <= 0x7FFFFFFF or int(b) not in PNG_BITS_PER_PIXEL or int(il) not in (0, 1):
            raise ValueError(name + ": 1 <= width, height <= 2^31 - 1, bits_per_pixel in %r, interlace 0 or 1 and non-null device pointers "
                             "are required" % (PNG_BITS_PER_PIXEL,))
        total_rows += sum(png_idat_layout(int(w), int(h), int(b), 1)[2]) if int(il) else int(h)
    if total_rows > 0x7FFFFFFF:
        raise ValueError(name + ": more than 2^31 - 1 rows in one call")
    return n


def png_adam7_merge_batch_device(engine, pass_ptrs, widths, heights, bits_per_pixel, out_ptrs, stream=None):
    """The Adam7 interleave of many device-resident images in one launch (zs_png_adam7_merge_batch_device): pass_ptrs[i] holds
    image i's reconstructed passes back to back (png_idat_layout gives their sizes; no filter bytes), out_ptrs[i] receives
    heights[i] rows of ceil(widths[i] * bits_per_pixel[i] / 8) bytes."""
    n = _png_image_check("png_adam7_merge_batch_device", pass_ptrs, widths, heights, bits_per_pixel, [0] * len(pass_ptrs), out_ptrs)
    if n == 0:
        return
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    rc = _native.lib().zs_png_adam7_merge_batch_device(engine.handle, n, VP(*[int(p) for p in pass_ptrs]), I64(*[int(x) for x in widths]),
                                                       I64(*[int(x) for x in heights]), I32(*[int(x) for x in bits_per_pixel]),
                                                       VP(*[int(p) for p in out_ptrs]), ctypes.c_void_p(stream or 0))
    if rc != 0:
        raise ValueError("zs_png_adam7_merge_batch_device failed (%d): %s" % (rc, engine.last_error()))


def png_decode_batch_device(engine, idat_ptrs, idat_lens, widths, heights, bits_per_pixel, interlace, out_ptrs, stream=None):
    """IDAT payloads -> raw scanline pixels for many device-resident PNG images in one call (zs_png_decode_batch_device):
    inflate, reconstruction and, for interlace[i] = 1, the Adam7 interleave, nothing leaving the device.  idat_ptrs[i] /
    idat_lens[i]: the image's IDAT data concatenated (one zlib stream).  Returns a status per image: 0, or -3
    (ZS_DATA_ERROR) for an image whose stream does not inflate, has the wrong length or holds a filter type above 4
    (engine.last_error() names the first such image; the others are decoded all the same)."""
    if len(idat_lens) != len(idat_ptrs):
        raise ValueError("png_decode_batch_device: the argument lists differ in length")
    n = _png_image_check("png_decode_batch_device", idat_ptrs, widths, heights, bits_per_pixel, interlace, out_ptrs)
    if any(not 0 <= int(x) <= 0x7FFFFFFF - 1024 for x in idat_lens):
        raise ValueError("png_decode_batch_device: a stream's length is negative or above 2 GiB - 1 KiB")
    if n == 0:
        return []
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    status = I32()
    rc = _native.lib().zs_png_decode_batch_device(engine.handle, n, VP(*[int(p) for p in idat_ptrs]), I64(*[int(x) for x in idat_lens]),
                                                  I64(*[int(x) for x in widths]), I64(*[int(x) for x in heights]),
                                                  I32(*[int(x) for x in bits_per_pixel]), I32(*[int(x) for x in interlace]),
                                                  VP(*[int(p) for p in out_ptrs]), status, ctypes.c_void_p(stream or 0))
    if rc not in (0, -3):
        raise ValueError("zs_png_decode_batch_device failed (%d): %s" % (rc, engine.last_error()))
    return list(status)


CRC32_TILE = 8192          # bytes of a span one wave takes at a time (zs_crc32.h kCrcTile)
CRC32_TILES_PER_WG = 4     # tiles a workgroup takes in one pass (kCrcWaves)
_CRC_MAX_LEN = 0x7FFFFFFF - 1024
# PNG specification table 11.1: color type -> (channels, bit depths)
PNG_COLOR_TYPES = {0: (1, (1, 2, 4, 8, 16)), 2: (3, (8, 16)), 3: (1, (1, 2, 4, 8)), 4: (2, (8, 16)), 6: (4, (8, 16))}


def crc32_device(engine, ptr, length, seed=0, stream=None):
    """zlib.crc32(bytes, seed) of a device-resident buffer of any alignment (zs_crc32_device): seed 0 starts a CRC, a result
    fed back as the seed continues it."""
    length, seed = int(length), int(seed)
    if not 0 <= length <= _CRC_MAX_LEN or not 0 <= seed <= 0xFFFFFFFF or (length > 0 and not ptr):
        raise ValueError("crc32_device: 0 <= length <= 2 GiB - 1 KiB, a 32-bit seed and a non-null device pointer are required")
    out = ctypes.c_uint32(0)
    rc = _native.lib().zs_crc32_device(engine.handle, ctypes.c_void_p(ptr or 0), length, seed, ctypes.byref(out), ctypes.c_void_p(stream or 0))
    if rc != 0:
        raise ValueError("zs_crc32_device failed (%d): %s" % (rc, engine.last_error()))
    return int(out.value)


def crc32_batch_device(engine, ptrs, lengths, seeds=None, stream=None):
    """crc32_device for many spans of any lengths in one launch (zs_crc32_batch_device) -> the CRCs in input order.
    seeds: None (all 0) or one per span."""
    n = len(ptrs)
    if len(lengths) != n or (seeds is not None and len(seeds) != n):
        raise ValueError("crc32_batch_device: the argument lists differ in length")
    for p, ln in zip(ptrs, lengths):
        if not 0 <= int(ln) <= _CRC_MAX_LEN or (int(ln) > 0 and not p):
            raise ValueError("crc32_batch_device: 0 <= length <= 2 GiB - 1 KiB and non-null device pointers are required")
    if seeds is not None and any(not 0 <= int(s) <= 0xFFFFFFFF for s in seeds):
        raise ValueError("crc32_batch_device: a seed is not a 32-bit value")
    if n == 0:
        return []
    out = (ctypes.c_uint32 * n)()
    rc = _native.lib().zs_crc32_batch_device(engine.handle, n, (ctypes.c_void_p * n)(*[int(p or 0) for p in ptrs]),
                                             (ctypes.c_int64 * n)(*[int(x) for x in lengths]),
                                             (ctypes.c_uint32 * n)(*[int(s) for s in seeds]) if seeds is not None else None, out,
                                             ctypes.c_void_p(stream or 0))
    if rc != 0:
        raise ValueError("zs_crc32_batch_device failed (%d): %s" % (rc, engine.last_error()))
    return [int(v) for v in out]


def png_file_bound(idat_len, idat_chunk_bytes=0, extra_len=0):
    """zs_png_file_bound (host code, no GPU): bytes of the PNG file around a zlib stream of idat_len bytes in IDAT chunks of at
    most idat_chunk_bytes data bytes (0: one chunk) with extra_len bytes of caller chunks.  ValueError for bad arguments."""
    idat_len, idat_chunk_bytes, extra_len = int(idat_len), int(idat_chunk_bytes), int(extra_len)
    ok = 0 <= idat_len < 1 << 60 and 0 <= extra_len < 1 << 60 and 0 <= idat_chunk_bytes <= 0x7FFFFFFF
    v = _native.lib().zs_png_file_bound(idat_len, idat_chunk_bytes, extra_len) if ok else -1
    if v < 0:
        raise ValueError("png_file_bound: non-negative lengths and 0 <= idat_chunk_bytes <= 2^31 - 1 are required (one chunk holds 2^31 - 1 bytes)")
    return int(v)


def _png_chunks_well_formed(b):
    at = 0
    while at < len(b):
        if len(b) - at < 12:
            return False
        n = int.from_bytes(b[at:at + 4], "big")
        if n > 0x7FFFFFFF or n > len(b) - at - 12:
            return False
        at += 12 + n
    return True


def _png_encode_files(name, engine, pixel_ptrs, widths, heights, bit_depths, color_types, filters, interlace, out_ptrs, out_caps, extra, rows_per_write,
                      idat_chunk_bytes, level, strategy, hash_variant, stream, return_status):
    """The one body of png_encode_batch_device (interlace False: zs_png_encode_batch_device) and png_encode_interlace_batch_device
    (interlace None or a list: zs_png_encode_interlace_batch_device): the argument checks, the extra chunks and the error
    mapping."""
    n = len(pixel_ptrs)
    with_interlace = interlace is not False
    if not with_interlace or interlace is None:
        interlace = [0] * n
    if not (len(widths) == len(heights) == len(bit_depths) == len(color_types) == len(filters) == len(out_ptrs) == len(out_caps) == len(interlace) == n) or \
            (extra is not None and len(extra) != n):
        raise ValueError(name + ": the argument lists differ in length")
    if int(rows_per_write) < 0 or not 0 <= int(idat_chunk_bytes) <= 0x7FFFFFFF:
        raise ValueError(name + ": rows_per_write >= 0 and 0 <= idat_chunk_bytes <= 2^31 - 1 are required")
    if not -1 <= int(level) <= 9 or not 0 <= int(strategy) <= 4:
        raise ValueError(name + ": level -1..9 and strategy 0..4 are required")
    total_rows = 0
    for p, w, h, bd, ct, f, il, o, cap in zip(pixel_ptrs, widths, heights, bit_depths, color_types, filters, interlace, out_ptrs, out_caps):
        if not p or not o or not 1 <= int(w) <= 0x7FFFFFFF or not 1 <= int(h) <= 0x7FFFFFFF or not 0 <= int(f) <= 5 or int(cap) < 0 or int(il) not in (0, 1):
            raise ValueError(name + ": 1 <= width, height <= 2^31 - 1, filter 0..5%s and non-null device pointers are required" %
                             (", interlace 0 or 1" if with_interlace else ""))
        if int(ct) not in PNG_COLOR_TYPES or int(bd) not in PNG_COLOR_TYPES[int(ct)][1]:
            raise ValueError(name + ": color type %r with bit depth %r is not in PNG specification table 11.1" % (ct, bd))
        bits = int(bd) * PNG_COLOR_TYPES[int(ct)][0]
        if int(il):
            total, _, rows = png_idat_layout(w, h, bits, 1)
            rows = sum(rows)
        else:
            total, rows = int(h) * ((int(w) * bits + 7) // 8 + 1), int(h)
        if total > _CRC_MAX_LEN:
            raise ValueError(name + ": a filtered image is above 2 GiB - 1 KiB")
        total_rows += rows
    if total_rows > 0x7FFFFFFF:
        raise ValueError(name + ": more than 2^31 - 1 rows in one call")
    if extra is not None:
        extra = [bytes(x) if x is not None else b"" for x in extra]
        if not all(_png_chunks_well_formed(x) for x in extra):
            raise ValueError(name + ": an image's extra chunks are not a sequence of whole chunks")
    if n == 0:
        return (0, [], []) if return_status else []
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status = I64(), I32()
    # (the bytes objects are read in place: they outlive the call)
    x_ptr = VP(*[ctypes.cast(ctypes.c_char_p(x), ctypes.c_void_p).value if x else None for x in extra]) if extra is not None else None
    x_len = I64(*[len(x) for x in extra]) if extra is not None else None
    head = (engine.handle, n, VP(*[int(p) for p in pixel_ptrs]), I64(*[int(x) for x in widths]), I64(*[int(x) for x in heights]),
            I32(*[int(x) for x in bit_depths]), I32(*[int(x) for x in color_types]), I32(*[int(x) for x in filters]))
    tail = (x_ptr, x_len, int(rows_per_write), int(idat_chunk_bytes), VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), out_len, status,
            int(level), int(strategy), int(hash_variant), ctypes.c_void_p(stream or 0))
    if with_interlace:
        rc = _native.lib().zs_png_encode_interlace_batch_device(*head, I32(*[int(x) for x in interlace]), *tail)
    else:
        rc = _native.lib().zs_png_encode_batch_device(*head, *tail)
    if return_status:
        return rc, list(out_len), list(status)
    if rc != 0:
        raise ZlibStreamException("png encode: " + engine.last_error())
    return list(out_len)


def png_encode_batch_device(engine, pixel_ptrs, widths, heights, bit_depths, color_types, filters, out_ptrs, out_caps, extra=None,
                            rows_per_write=1, idat_chunk_bytes=0, level=6, strategy=0, hash_variant=0, stream=None, return_status=False):
    """Pixels -> complete PNG files for many device-resident images in one call (zs_png_encode_batch_device): the zlib stream
    of png_idat_batch_device (same filters, rows_per_write, level, strategy) cut into IDAT chunks of at most idat_chunk_bytes
    data bytes (0: one chunk), between signature + IHDR + extra[i] and IEND.  pixel_ptrs[i]: heights[i] rows of
    ceil(widths[i] * bit_depths[i] * channels / 8) bytes; extra: None or one bytes object per image of chunks framed already
    (PLTE, tRNS, ...), written verbatim behind IHDR.  Returns the file lengths; return_status: (rc, lengths, statuses), -5
    (ZS_BUF_ERROR) for an image whose out_caps entry is below its file's length."""
    return _png_encode_files("png_encode_batch_device", engine, pixel_ptrs, widths, heights, bit_depths, color_types, filters, False, out_ptrs, out_caps, extra,
                             rows_per_write, idat_chunk_bytes, level, strategy, hash_variant, stream, return_status)


def png_adam7_split_batch_device(engine, pixel_ptrs, widths, heights, bits_per_pixel, pass_ptrs, stream=None):
    """The Adam7 split of many device-resident images in one launch (zs_png_adam7_split_batch_device), the exact inverse of
    png_adam7_merge_batch_device: pixel_ptrs[i] holds heights[i] rows of ceil(widths[i] * bits_per_pixel[i] / 8) bytes,
    pass_ptrs[i] receives the present passes back to back (png_idat_layout gives their sizes; no filter bytes).  At 1, 2 and
    4 bits the unused low bits of a pass row's last byte are zero whatever the input's padding bits hold."""
    n = len(pixel_ptrs)
    if not (len(widths) == len(heights) == len(bits_per_pixel) == len(pass_ptrs) == n):
        raise ValueError("png_adam7_split_batch_device: the argument lists differ in length")
    _png_image_check("png_adam7_split_batch_device", pixel_ptrs, widths, heights, bits_per_pixel, [1] * n, pass_ptrs)
    if n == 0:
        return
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    rc = _native.lib().zs_png_adam7_split_batch_device(engine.handle, n, VP(*[int(p) for p in pixel_ptrs]), I64(*[int(x) for x in widths]),
                                                       I64(*[int(x) for x in heights]), I32(*[int(x) for x in bits_per_pixel]),
                                                       VP(*[int(p) for p in pass_ptrs]), ctypes.c_void_p(stream or 0))
    if rc != 0:
        raise ValueError("zs_png_adam7_split_batch_device failed (%d): %s" % (rc, engine.last_error()))


def png_idat_interlace_batch_device(engine, pixel_ptrs, widths, heights, bits_per_pixel, interlace, filters, out_ptrs, out_caps, rows_per_write=1,
                                    level=6, strategy=0, hash_variant=0, stream=None, return_status=False):
    """Pixels -> IDAT payloads, interlaced (Adam7) or not, for many device-resident images in one call
    (zs_png_idat_interlace_batch_device).  interlace: None (all 0) or 0 / 1 per image.  An image with interlace 0 gets the
    stream of png_idat_batch_device; one with interlace 1 is split into its passes on the device, every present pass is
    filtered on its own with filters[i], and the filtered passes back to back are the stream's input.  rows_per_write counts
    rows of the stream in stream order (pass rows for an interlaced image; a Write may span a pass boundary).  Returns the
    stream lengths; return_status as Engine.deflate_writes_batch_device."""
    name = "png_idat_interlace_batch_device"
    n = len(pixel_ptrs)
    if interlace is None:
        interlace = [0] * n
    if not (len(filters) == len(out_caps) == n):
        raise ValueError(name + ": the argument lists differ in length")
    _png_image_check(name, pixel_ptrs, widths, heights, bits_per_pixel, interlace, out_ptrs)
    if any(not 0 <= int(f) <= 5 for f in filters) or int(rows_per_write) < 0:
        raise ValueError(name + ": filter 0..5 and rows_per_write >= 0 are required")
    if not -1 <= int(level) <= 9 or not 0 <= int(strategy) <= 4:
        raise ValueError(name + ": level -1..9 and strategy 0..4 are required")
    for w, h, b, il in zip(widths, heights, bits_per_pixel, interlace):
        if png_idat_layout(w, h, b, il)[0] > _CRC_MAX_LEN:
            raise ValueError(name + ": a filtered image is above 2 GiB - 1 KiB")
    if n == 0:
        return (0, [], []) if return_status else []
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status = I64(), I32()
    rc = _native.lib().zs_png_idat_interlace_batch_device(engine.handle, n, VP(*[int(p) for p in pixel_ptrs]), I64(*[int(x) for x in widths]),
                                                          I64(*[int(x) for x in heights]), I32(*[int(x) for x in bits_per_pixel]),
                                                          I32(*[int(x) for x in interlace]), I32(*[int(x) for x in filters]), int(rows_per_write),
                                                          VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), out_len, status,
                                                          int(level), int(strategy), int(hash_variant), ctypes.c_void_p(stream or 0))
    if return_status:
        return rc, list(out_len), list(status)
    if rc != 0:
        raise ZlibStreamException("deflating: " + engine.last_error())
    return list(out_len)


def png_encode_interlace_batch_device(engine, pixel_ptrs, widths, heights, bit_depths, color_types, filters, out_ptrs, out_caps, interlace=None,
                                      extra=None, rows_per_write=1, idat_chunk_bytes=0, level=6, strategy=0, hash_variant=0, stream=None,
                                      return_status=False):
    """png_encode_batch_device with IHDR's interlace byte per image (zs_png_encode_interlace_batch_device): interlace None (all 0)
    or 0 / 1 per image; the IDAT chunks hold the stream of png_idat_interlace_batch_device.  With interlace None or all 0 the
    files are png_encode_batch_device's byte for byte.  png_file_bound(deflate_bound(png_idat_layout(w, h, bits, interlace)[0]),
    idat_chunk_bytes, len(extra[i])) is always enough room."""
    return _png_encode_files("png_encode_interlace_batch_device", engine, pixel_ptrs, widths, heights, bit_depths, color_types, filters, interlace, out_ptrs,
                             out_caps, extra, rows_per_write, idat_chunk_bytes, level, strategy, hash_variant, stream, return_status)


_PNG_INFO_FIELDS = ("width", "height", "bit_depth", "color_type", "interlace", "bits_per_pixel", "idat_bytes", "pixel_bytes", "n_idat")


def png_file_info(data):
    """zs_png_file_info (host code, no GPU, no engine): the chunk walk of one PNG file given as bytes -> a dict of width,
    height, bit_depth, color_type, interlace, bits_per_pixel, idat_bytes, pixel_bytes, n_idat.  ZlibStreamException for a
    file that is not a whole PNG: bad signature, truncated chunk, IHDR missing / not first / out of specification, no IDAT,
    IDAT chunks not consecutive, missing IEND, a wrong CRC in IHDR, PLTE, IDAT or IEND (ancillary chunks are not verified)."""
    data = bytes(data)
    info = _native.PngInfo()
    rc = _native.lib().zs_png_file_info(data, len(data), ctypes.byref(info))
    if rc != 0:
        raise ZlibStreamException("png_file_info: not a whole PNG file (%d)" % rc)
    return {k: int(getattr(info, k)) for k in _PNG_INFO_FIELDS}


def png_decode_files_batch(engine, files, out_ptrs, out_caps, stream=None):
    """PNG files (bytes objects in host memory) -> raw scanline pixels in device buffers, many files a call
    (zs_png_decode_files_batch): the chunk walk on the host, one upload, the critical chunks' CRC-32 and the gather of the
    IDAT data on the device, then inflate, reconstruction and the Adam7 interleave.  Returns (statuses, infos): 0, -5
    (ZS_BUF_ERROR: out_caps[i] below the image's pixel_bytes) or -3 (ZS_DATA_ERROR; engine.last_error() names the first
    failing file and the reason; the other files are decoded all the same), and one png_file_info dict per file."""
    n = len(files)
    if len(out_ptrs) != n or len(out_caps) != n:
        raise ValueError("png_decode_files_batch: the argument lists differ in length")
    if any(not o or int(cap) < 0 for o, cap in zip(out_ptrs, out_caps)):
        raise ValueError("png_decode_files_batch: non-null device pointers and non-negative capacities are required")
    if n == 0:
        return [], []
    files = [bytes(f) for f in files]
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    info, status = (_native.PngInfo * n)(), I32()
    rc = _native.lib().zs_png_decode_files_batch(engine.handle, n, VP(*[ctypes.cast(ctypes.c_char_p(f), ctypes.c_void_p).value for f in files]),  # (read in place)
                                                 I64(*[len(f) for f in files]),
                                                 VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), info, status,
                                                 ctypes.c_void_p(stream or 0))
    if rc not in (0, -3, -5):
        raise ValueError("zs_png_decode_files_batch failed (%d): %s" % (rc, engine.last_error()))
    return list(status), [{k: int(getattr(i, k)) for k in _PNG_INFO_FIELDS} for i in info]


PNG_RGBA8, PNG_RGBA16 = 0, 1  # ZS_PNG_RGBA8 / ZS_PNG_RGBA16: 4 bytes a pixel, or four uint16 in host order


def _host_ptr(b):
    return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value if b else None


def png_expand_batch_device(engine, in_ptrs, widths, heights, bit_depths, color_types, out_ptrs, plte=None, trns=None, format=PNG_RGBA8,
                            stream=None):
    """Raw scanlines -> RGBA pixels for many device-resident images in one launch (zs_png_expand_batch_device): every legal
    (color type, bit depth) pair to rows of widths[i] * 4 bytes (PNG_RGBA8) or widths[i] * 4 uint16 (PNG_RGBA16), PLTE and tRNS
    applied.  plte / trns: None, or one entry per image -- the chunk's data as bytes, or None (plte is required at color type
    3; trns holds 2 bytes at type 0, 6 at type 2, 1 .. the PLTE's entries at type 3; both are ignored at types 4 and 6).
    out_ptrs[i] must be aligned to a pixel (4 or 8 bytes) and must not overlap in_ptrs[i]."""
    n = len(in_ptrs)
    if not (len(widths) == len(heights) == len(bit_depths) == len(color_types) == len(out_ptrs) == n) or \
            (plte is not None and len(plte) != n) or (trns is not None and len(trns) != n):
        raise ValueError("png_expand_batch_device: the argument lists differ in length")
    if format not in (PNG_RGBA8, PNG_RGBA16):
        raise ValueError("png_expand_batch_device: format is PNG_RGBA8 or PNG_RGBA16")
    px = 8 if format == PNG_RGBA16 else 4
    plte = [bytes(x) if x is not None else b"" for x in plte] if plte is not None else [b""] * n
    trns = [bytes(x) if x is not None else b"" for x in trns] if trns is not None else [b""] * n
    for p, w, h, bd, ct, o, pl, tr in zip(in_ptrs, widths, heights, bit_depths, color_types, out_ptrs, plte, trns):
        if not p or not o or int(o) % px or not 1 <= int(w) <= 0x7FFFFFFF or not 1 <= int(h) <= 0x7FFFFFFF:
            raise ValueError("png_expand_batch_device: 1 <= width, height <= 2^31 - 1, non-null device pointers and outputs aligned to a pixel are required")
        if int(ct) not in PNG_COLOR_TYPES or int(bd) not in PNG_COLOR_TYPES[int(ct)][1]:
            raise ValueError("png_expand_batch_device: color type %r with bit depth %r is not in PNG specification table 11.1" % (ct, bd))
        if int(ct) == 3 and (len(pl) % 3 or not 3 <= len(pl) <= 768 or len(tr) > len(pl) // 3):
            raise ValueError("png_expand_batch_device: a palette image needs a PLTE of 1 .. 256 entries and a tRNS no longer than it")
        if int(ct) in (0, 2) and len(tr) not in (0, 2 if int(ct) == 0 else 6):
            raise ValueError("png_expand_batch_device: a tRNS holds 2 bytes at color type 0 and 6 at color type 2")
    if sum(int(h) for h in heights) > 0x7FFFFFFF:
        raise ValueError("png_expand_batch_device: more than 2^31 - 1 rows in one call")
    if n == 0:
        return
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    # (the bytes objects are read in place: they outlive the call)
    rc = _native.lib().zs_png_expand_batch_device(engine.handle, n, VP(*[int(p) for p in in_ptrs]), I64(*[int(x) for x in widths]),
                                                  I64(*[int(x) for x in heights]), I32(*[int(x) for x in bit_depths]),
                                                  I32(*[int(x) for x in color_types]), VP(*[_host_ptr(x) for x in plte]),
                                                  I32(*[len(x) // 3 for x in plte]), VP(*[_host_ptr(x) for x in trns]),
                                                  I32(*[len(x) if int(ct) in (0, 2, 3) else 0 for x, ct in zip(trns, color_types)]), int(format),
                                                  VP(*[int(p) for p in out_ptrs]), ctypes.c_void_p(stream or 0))
    if rc != 0:
        raise ValueError("zs_png_expand_batch_device failed (%d): %s" % (rc, engine.last_error()))


def png_file_colors(data):
    """zs_png_file_colors (host code, no GPU, no engine): png_file_info's walk and checks, and the data bytes of the file's PLTE
    and tRNS chunks -> (plte, trns), b"" where the file has none or the chunk means nothing at its color type (a tRNS at
    types 4 and 6, a PLTE at types 0 and 4).  ZlibStreamException for what png_file_info rejects and for a PLTE or tRNS of a
    wrong length, a second one, one behind IDAT, a palette image without PLTE or with its tRNS in front of it, a tRNS whose
    CRC is wrong."""
    data = bytes(data)
    plte, trns = (ctypes.c_uint8 * 768)(), (ctypes.c_uint8 * 256)()
    n_plte, n_trns = ctypes.c_int(0), ctypes.c_int(0)
    rc = _native.lib().zs_png_file_colors(data, len(data), plte, ctypes.byref(n_plte), trns, ctypes.byref(n_trns))
    if rc != 0:
        raise ZlibStreamException("png_file_colors: not a whole PNG file, or its PLTE / tRNS chunks break the rules (%d)" % rc)
    return bytes(plte[:3 * n_plte.value]), bytes(trns[:n_trns.value])


def png_decode_files_rgba_batch(engine, files, out_ptrs, out_caps, format=PNG_RGBA8, stream=None):
    """PNG files (bytes objects in host memory) -> RGBA pixels in device buffers, many files a call
    (zs_png_decode_files_rgba_batch): png_decode_files_batch into a buffer of the engine with png_expand_batch_device behind it,
    the files' own PLTE and tRNS applied.  out_ptrs[i] receives width * height * 4 bytes (PNG_RGBA8) or * 8 (PNG_RGBA16) and
    must be aligned to a pixel.  Returns (statuses, infos) like png_decode_files_batch: 0, -5 (ZS_BUF_ERROR: out_caps[i] is
    below that size) or -3 (ZS_DATA_ERROR; engine.last_error() names the first failing file and the reason)."""
    n = len(files)
    if len(out_ptrs) != n or len(out_caps) != n:
        raise ValueError("png_decode_files_rgba_batch: the argument lists differ in length")
    if format not in (PNG_RGBA8, PNG_RGBA16):
        raise ValueError("png_decode_files_rgba_batch: format is PNG_RGBA8 or PNG_RGBA16")
    if any(not o or int(o) % (8 if format == PNG_RGBA16 else 4) or int(cap) < 0 for o, cap in zip(out_ptrs, out_caps)):
        raise ValueError("png_decode_files_rgba_batch: non-null device pointers aligned to a pixel and non-negative capacities are required")
    if n == 0:
        return [], []
    files = [bytes(f) for f in files]
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    info, status = (_native.PngInfo * n)(), I32()
    rc = _native.lib().zs_png_decode_files_rgba_batch(engine.handle, n, VP(*[_host_ptr(f) for f in files]),  # (read in place)
                                                      I64(*[len(f) for f in files]), int(format),
                                                      VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), info, status,
                                                      ctypes.c_void_p(stream or 0))
    if rc not in (0, -3, -5):
        raise ValueError("zs_png_decode_files_rgba_batch failed (%d): %s" % (rc, engine.last_error()))
    return list(status), [{k: int(getattr(i, k)) for k in _PNG_INFO_FIELDS} for i in info]


def png_pack_batch_device(engine, in_ptrs, widths, heights, bit_depths, color_types, out_ptrs, plte=None, trns=None, format=PNG_RGBA8,
                          stream=None, return_unmatched=False):
    """RGBA pixels -> raw scanlines for many device-resident images in one launch (zs_png_pack_batch_device), the inverse of
    png_expand_batch_device: in_ptrs[i] holds heights[i] rows of widths[i] * 4 bytes (PNG_RGBA8) or widths[i] * 4 uint16
    (PNG_RGBA16) and must be aligned to a pixel; out_ptrs[i] receives rows of ceil(widths[i] * bits / 8) bytes at any
    alignment.  plte / trns as for png_expand_batch_device.  A palette pixel with no equal entry gets index 0;
    return_unmatched: the list of their counts per image (0 for the other color types) -- the call then waits for it."""
    name = "png_pack_batch_device"
    n = len(in_ptrs)
    if not (len(widths) == len(heights) == len(bit_depths) == len(color_types) == len(out_ptrs) == n) or \
            (plte is not None and len(plte) != n) or (trns is not None and len(trns) != n):
        raise ValueError(name + ": the argument lists differ in length")
    if format not in (PNG_RGBA8, PNG_RGBA16):
        raise ValueError(name + ": format is PNG_RGBA8 or PNG_RGBA16")
    px = 8 if format == PNG_RGBA16 else 4
    plte = [bytes(x) if x is not None else b"" for x in plte] if plte is not None else [b""] * n
    trns = [bytes(x) if x is not None else b"" for x in trns] if trns is not None else [b""] * n
    for p, w, h, bd, ct, o, pl, tr in zip(in_ptrs, widths, heights, bit_depths, color_types, out_ptrs, plte, trns):
        if not p or not o or int(p) % px or not 1 <= int(w) <= 0x7FFFFFFF or not 1 <= int(h) <= 0x7FFFFFFF:
            raise ValueError(name + ": 1 <= width, height <= 2^31 - 1, non-null device pointers and inputs aligned to a pixel are required")
        if int(ct) not in PNG_COLOR_TYPES or int(bd) not in PNG_COLOR_TYPES[int(ct)][1]:
            raise ValueError(name + ": color type %r with bit depth %r is not in PNG specification table 11.1" % (ct, bd))
        if int(ct) == 3 and (len(pl) % 3 or not 3 <= len(pl) <= 768 or len(tr) > len(pl) // 3):
            raise ValueError(name + ": a palette image needs a PLTE of 1 .. 256 entries and a tRNS no longer than it")
        if int(ct) in (0, 2) and len(tr) not in (0, 2 if int(ct) == 0 else 6):
            raise ValueError(name + ": a tRNS holds 2 bytes at color type 0 and 6 at color type 2")
    if sum(int(h) for h in heights) > 0x7FFFFFFF:
        raise ValueError(name + ": more than 2^31 - 1 rows in one call")
    if n == 0:
        return [] if return_unmatched else None
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    unmatched = I64() if return_unmatched else None
    # (the bytes objects are read in place: they outlive the call)
    rc = _native.lib().zs_png_pack_batch_device(engine.handle, n, VP(*[int(p) for p in in_ptrs]), I64(*[int(x) for x in widths]),
                                                I64(*[int(x) for x in heights]), I32(*[int(x) for x in bit_depths]),
                                                I32(*[int(x) for x in color_types]), VP(*[_host_ptr(x) for x in plte]),
                                                I32(*[len(x) // 3 for x in plte]), VP(*[_host_ptr(x) for x in trns]),
                                                I32(*[len(x) if int(ct) in (0, 2, 3) else 0 for x, ct in zip(trns, color_types)]), int(format),
                                                VP(*[int(p) for p in out_ptrs]), unmatched, ctypes.c_void_p(stream or 0))
    if rc != 0:
        raise ValueError("zs_png_pack_batch_device failed (%d): %s" % (rc, engine.last_error()))
    return [int(v) for v in unmatched] if return_unmatched else None


_PNG_SURVEY_FLAGS = ("opaque", "gray", "low8", "sample_depth", "n_colors")


def _survey_dict(s):
    d = {k: int(getattr(s, k)) for k in _PNG_SURVEY_FLAGS}
    d["colors"] = [tuple(s.colors[k]) for k in range(d["n_colors"] if d["n_colors"] <= 256 else 0)]
    return d


def _survey_struct(d):
    s = _native.PngSurvey()
    for k in _PNG_SURVEY_FLAGS:
        setattr(s, k, int(d[k]))
    for k, c in enumerate(d.get("colors", ())[:256]):
        for j in range(4):
            s.colors[k][j] = int(c[j])
    return s


def png_survey_batch_device(engine, in_ptrs, widths, heights, format=PNG_RGBA8, stream=None):
    """What the pixels of many device-resident RGBA images allow (zs_png_survey_batch_device): one dict per image of opaque,
    gray, low8 (0 / 1), sample_depth (1, 2, 4, 8; 16 where low8 is 0), n_colors (1 .. 256, or 257 for more, and where low8 is
    0) and colors, the n_colors distinct (R, G, B, A) tuples at 8 bits ascending by (A, R, G, B) (empty at 257).  in_ptrs[i]
    as for png_pack_batch_device.  The same on every run."""
    name = "png_survey_batch_device"
    n = len(in_ptrs)
    if not (len(widths) == len(heights) == n):
        raise ValueError(name + ": the argument lists differ in length")
    if format not in (PNG_RGBA8, PNG_RGBA16):
        raise ValueError(name + ": format is PNG_RGBA8 or PNG_RGBA16")
    px = 8 if format == PNG_RGBA16 else 4
    for p, w, h in zip(in_ptrs, widths, heights):
        if not p or int(p) % px or not 1 <= int(w) <= 0x7FFFFFFF or not 1 <= int(h) <= 0x7FFFFFFF:
            raise ValueError(name + ": 1 <= width, height <= 2^31 - 1 and non-null device pointers aligned to a pixel are required")
    if sum(int(h) for h in heights) > 0x7FFFFFFF:
        raise ValueError(name + ": more than 2^31 - 1 rows in one call")
    if n == 0:
        return []
    VP, I64 = ctypes.c_void_p * n, ctypes.c_int64 * n
    out = (_native.PngSurvey * n)()
    rc = _native.lib().zs_png_survey_batch_device(engine.handle, n, VP(*[int(p) for p in in_ptrs]), I64(*[int(x) for x in widths]),
                                                  I64(*[int(x) for x in heights]), int(format), out, ctypes.c_void_p(stream or 0))
    if rc != 0:
        raise ValueError("zs_png_survey_batch_device failed (%d): %s" % (rc, engine.last_error()))
    return [_survey_dict(s) for s in out]


def png_choose_format(survey):
    """zs_png_choose_format (host code, no GPU, no engine): a survey dict (opaque, gray, low8, sample_depth, n_colors) ->
    (color_type, bit_depth).  The rule compares bits per pixel -- a palette only where its depth is strictly below the
    base's -- and does not promise the smallest file.  ValueError for a sample_depth or n_colors outside their values."""
    try:
        d = {k: int(survey[k]) for k in _PNG_SURVEY_FLAGS}
    except (KeyError, TypeError, ValueError):
        raise ValueError("png_choose_format: a survey holds opaque, gray, low8, sample_depth and n_colors")
    if d["sample_depth"] not in (1, 2, 4, 8, 16) or (d["sample_depth"] == 16) != (not d["low8"]) or not 1 <= d["n_colors"] <= 257:
        raise ValueError("png_choose_format: sample_depth is 1, 2, 4 or 8 (16 exactly where low8 is 0) and n_colors 1 .. 257")
    ct, bd = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _native.lib().zs_png_choose_format(ctypes.byref(_survey_struct(d)), ctypes.byref(ct), ctypes.byref(bd))
    if rc != 0:
        raise ValueError("zs_png_choose_format failed (%d)" % rc)
    return ct.value, bd.value


def png_encode_rgba_batch_device(engine, pixel_ptrs, widths, heights, filters, out_ptrs, out_caps, format=PNG_RGBA8, interlace=None, extra=None,
                                 rows_per_write=1, idat_chunk_bytes=0, level=6, strategy=0, hash_variant=0, stream=None, return_status=False):
    """RGBA pixels -> complete PNG files for many device-resident images in one call (zs_png_encode_rgba_batch_device): the
    survey, png_choose_format per image, PLTE and tRNS for the palette images, the pack, then
    png_encode_interlace_batch_device's body -- the files are that call's byte for byte.  pixel_ptrs[i] / format as for
    png_pack_batch_device; the rest as for png_encode_interlace_batch_device, with extra[i] in front of PLTE (chunks that must
    follow PLTE are not supported).  png_file_bound(deflate_bound(png_idat_layout(w, h, 32 or 64, interlace)[0]),
    idat_chunk_bytes, len(extra[i]) + 1048) is always enough room.  Returns (lengths, color_types, bit_depths);
    return_status: (rc, lengths, statuses, color_types, bit_depths)."""
    name = "png_encode_rgba_batch_device"
    n = len(pixel_ptrs)
    if interlace is None:
        interlace = [0] * n
    if not (len(widths) == len(heights) == len(filters) == len(out_ptrs) == len(out_caps) == len(interlace) == n) or (extra is not None and len(extra) != n):
        raise ValueError(name + ": the argument lists differ in length")
    if format not in (PNG_RGBA8, PNG_RGBA16):
        raise ValueError(name + ": format is PNG_RGBA8 or PNG_RGBA16")
    px = 8 if format == PNG_RGBA16 else 4
    if int(rows_per_write) < 0 or not 0 <= int(idat_chunk_bytes) <= 0x7FFFFFFF:
        raise ValueError(name + ": rows_per_write >= 0 and 0 <= idat_chunk_bytes <= 2^31 - 1 are required")
    if not -1 <= int(level) <= 9 or not 0 <= int(strategy) <= 4:
        raise ValueError(name + ": level -1..9 and strategy 0..4 are required")
    total_rows = 0
    for p, w, h, f, il, o, cap in zip(pixel_ptrs, widths, heights, filters, interlace, out_ptrs, out_caps):
        if not p or not o or int(p) % px or not 1 <= int(w) <= 0x7FFFFFFF or not 1 <= int(h) <= 0x7FFFFFFF or not 0 <= int(f) <= 5 or int(cap) < 0 or \
                int(il) not in (0, 1):
            raise ValueError(name + ": 1 <= width, height <= 2^31 - 1, filter 0..5, interlace 0 or 1 and non-null device pointers, the pixels' aligned "
                             "to a pixel, are required")
        if int(w) * int(h) * px > _CRC_MAX_LEN:  # (held against the pixels as they come, whatever pair would be chosen)
            raise ValueError(name + ": a filtered image is above 2 GiB - 1 KiB")
        total, _, rows = png_idat_layout(w, h, 8 * px, int(il))
        if total > _CRC_MAX_LEN:
            raise ValueError(name + ": a filtered image is above 2 GiB - 1 KiB")
        total_rows += sum(rows)
    if total_rows > 0x7FFFFFFF:
        raise ValueError(name + ": more than 2^31 - 1 rows in one call")
    if extra is not None:
        extra = [bytes(x) if x is not None else b"" for x in extra]
        if not all(_png_chunks_well_formed(x) for x in extra):
            raise ValueError(name + ": an image's extra chunks are not a sequence of whole chunks")
    if n == 0:
        return (0, [], [], [], []) if return_status else ([], [], [])
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status, ct, bd = I64(), I32(), I32(), I32()
    # (the bytes objects are read in place: they outlive the call)
    x_ptr = VP(*[_host_ptr(x) for x in extra]) if extra is not None else None
    x_len = I64(*[len(x) for x in extra]) if extra is not None else None
    rc = _native.lib().zs_png_encode_rgba_batch_device(engine.handle, n, VP(*[int(p) for p in pixel_ptrs]), I64(*[int(x) for x in widths]),
                                                       I64(*[int(x) for x in heights]), int(format), I32(*[int(x) for x in filters]),
                                                       I32(*[int(x) for x in interlace]), x_ptr, x_len, int(rows_per_write), int(idat_chunk_bytes),
                                                       VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), out_len, status, ct, bd,
                                                       int(level), int(strategy), int(hash_variant), ctypes.c_void_p(stream or 0))
    if return_status:
        return rc, list(out_len), list(status), list(ct), list(bd)
    if rc != 0:
        raise ZlibStreamException("png encode: " + engine.last_error())
    return list(out_len), list(ct), list(bd)


PNG_DISPOSE_NONE, PNG_DISPOSE_BACKGROUND, PNG_DISPOSE_PREVIOUS = 0, 1, 2  # fcTL's dispose_op
PNG_BLEND_SOURCE, PNG_BLEND_OVER = 0, 1                                   # fcTL's blend_op
_PNG_FRAME_FIELDS = ("x", "y", "width", "height", "delay_num", "delay_den", "dispose_op", "blend_op", "data_bytes", "n_chunks")
_PNG_ANIM_FIELDS = ("animated", "n_frames", "n_plays", "default_is_frame")


def _anim_dict(a):
    d = {k: int(getattr(a.png, k)) for k in _PNG_INFO_FIELDS}
    d.update({k: int(getattr(a, k)) for k in _PNG_ANIM_FIELDS})
    return d


def png_anim_info(data):
    """zs_png_anim_info (host code, no GPU, no engine): the animation of one PNG file given as bytes -> (anim, frames): anim
    is png_file_info's dict plus animated, n_frames, n_plays and default_is_frame; frames one dict per frame of x, y, width,
    height, delay_num, delay_den, dispose_op, blend_op, data_bytes, n_chunks.  A file without an acTL is one frame: the whole
    canvas, dispose NONE, blend SOURCE.  Delays and n_plays are reported as the file holds them, never interpreted.
    ZlibStreamException for what png_file_info and png_file_colors reject and for acTL / fcTL / fdAT chunks that break the
    APNG specification's rules (include/zsgpu.h lists them)."""
    data = bytes(data)
    L = _native.lib()
    anim = _native.PngAnim()
    rc = L.zs_png_anim_info(data, len(data), ctypes.byref(anim), None, 0)
    if rc not in (0, -5):
        raise ZlibStreamException("png_anim_info: not a whole PNG file, or its acTL / fcTL / fdAT chunks break the rules (%d)" % rc)
    frames = (_native.PngFrame * anim.n_frames)()
    rc = L.zs_png_anim_info(data, len(data), ctypes.byref(anim), frames, anim.n_frames)
    if rc != 0:
        raise ZlibStreamException("png_anim_info failed (%d)" % rc)
    return _anim_dict(anim), [{k: int(getattr(f, k)) for k in _PNG_FRAME_FIELDS} for f in frames]


def png_compose_batch_device(engine, frame_ptrs, frames, widths, heights, out_ptrs, format=PNG_RGBA8, stream=None):
    """Frames -> canvases for many device-resident animations in one launch (zs_png_compose_batch_device).  frame_ptrs[i][f]:
    device pointer to frame f's own pixels (frames[i][f]["height"] rows of ["width"] * 4 or * 8 bytes, as
    png_expand_batch_device writes them); frames[i][f]: a dict with x, y, width, height, dispose_op, blend_op (png_anim_info's
    dicts do); out_ptrs[i] receives len(frames[i]) canvases of heights[i] * widths[i] * 4 (PNG_RGBA8) or * 8 (PNG_RGBA16)
    bytes back to back, canvas f being what a viewer shows while frame f is up.  Every pointer must be aligned to a pixel.
    Blend OVER is the APNG specification's integer arithmetic (include/zsgpu.h)."""
    n = len(frame_ptrs)
    if not (len(frames) == len(widths) == len(heights) == len(out_ptrs) == n) or any(len(p) != len(f) for p, f in zip(frame_ptrs, frames)):
        raise ValueError("png_compose_batch_device: the argument lists differ in length")
    if format not in (PNG_RGBA8, PNG_RGBA16):
        raise ValueError("png_compose_batch_device: format is PNG_RGBA8 or PNG_RGBA16")
    px = 8 if format == PNG_RGBA16 else 4
    for ptrs, frs, w, h, o in zip(frame_ptrs, frames, widths, heights, out_ptrs):
        if not o or int(o) % px or not 1 <= int(w) <= 0x7FFFFFFF or not 1 <= int(h) <= 0x7FFFFFFF or len(frs) < 1:
            raise ValueError("png_compose_batch_device: 1 <= width, height <= 2^31 - 1, at least one frame and outputs aligned to a pixel are required")
        for p, f in zip(ptrs, frs):
            if not p or int(p) % px:
                raise ValueError("png_compose_batch_device: a frame's pixels need a non-null device pointer aligned to a pixel")
            if f["x"] < 0 or f["y"] < 0 or f["width"] < 1 or f["height"] < 1 or f["x"] + f["width"] > int(w) or f["y"] + f["height"] > int(h):
                raise ValueError("png_compose_batch_device: a frame's region lies outside the canvas")
            if f["dispose_op"] not in (0, 1, 2) or f["blend_op"] not in (0, 1):
                raise ValueError("png_compose_batch_device: dispose_op is 0, 1 or 2 and blend_op 0 or 1")
    if sum(int(h) for h in heights) > 0x7FFFFFFF:
        raise ValueError("png_compose_batch_device: more than 2^31 - 1 canvas rows in one call")
    if n == 0:
        return
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    px_arrays = [(ctypes.c_void_p * len(p))(*[int(x) for x in p]) for p in frame_ptrs]
    fr_arrays = [(_native.PngFrame * len(frs))(*[_native.PngFrame(x=f["x"], y=f["y"], width=f["width"], height=f["height"], dispose_op=f["dispose_op"],
                                                                   blend_op=f["blend_op"]) for f in frs]) for frs in frames]
    rc = _native.lib().zs_png_compose_batch_device(engine.handle, n,
                                                   (ctypes.POINTER(ctypes.c_void_p) * n)(*[ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p)) for a in px_arrays]),
                                                   (ctypes.POINTER(_native.PngFrame) * n)(*[ctypes.cast(a, ctypes.POINTER(_native.PngFrame)) for a in fr_arrays]),
                                                   I32(*[len(f) for f in frames]), I64(*[int(x) for x in widths]), I64(*[int(x) for x in heights]),
                                                   int(format), VP(*[int(p) for p in out_ptrs]), ctypes.c_void_p(stream or 0))
    if rc != 0:
        raise ValueError("zs_png_compose_batch_device failed (%d): %s" % (rc, engine.last_error()))


def png_decode_anim_batch(engine, files, out_ptrs, out_caps, format=PNG_RGBA8, stream=None):
    """PNG files, animated or not (bytes objects in host memory) -> composed canvases in device buffers, many files a call
    (zs_png_decode_anim_batch): every frame of every file is one image of the batched decode, and one compose launch draws
    them.  out_ptrs[i] receives n_frames canvases of width * height * 4 bytes (PNG_RGBA8) or * 8 (PNG_RGBA16) back to back
    and must be aligned to a pixel.  Returns (statuses, anims): 0, -5 (ZS_BUF_ERROR: out_caps[i] below the canvases' size) or
    -3 (ZS_DATA_ERROR; engine.last_error() names the first failing file, the frame and the reason), and one png_anim_info
    dict per file.  One play's canvases are produced; delays and n_plays are the caller's to interpret (png_anim_info)."""
    n = len(files)
    if len(out_ptrs) != n or len(out_caps) != n:
        raise ValueError("png_decode_anim_batch: the argument lists differ in length")
    if format not in (PNG_RGBA8, PNG_RGBA16):
        raise ValueError("png_decode_anim_batch: format is PNG_RGBA8 or PNG_RGBA16")
    if any(not o or int(o) % (8 if format == PNG_RGBA16 else 4) or int(cap) < 0 for o, cap in zip(out_ptrs, out_caps)):
        raise ValueError("png_decode_anim_batch: non-null device pointers aligned to a pixel and non-negative capacities are required")
    if n == 0:
        return [], []
    files = [bytes(f) for f in files]
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    anim, status = (_native.PngAnim * n)(), I32()
    rc = _native.lib().zs_png_decode_anim_batch(engine.handle, n, VP(*[_host_ptr(f) for f in files]),  # (read in place)
                                                I64(*[len(f) for f in files]), int(format),
                                                VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), anim, status,
                                                ctypes.c_void_p(stream or 0))
    if rc not in (0, -3, -5):
        raise ValueError("zs_png_decode_anim_batch failed (%d): %s" % (rc, engine.last_error()))
    return list(status), [_anim_dict(a) for a in anim]


def _png_canvases_check(name, canvas_ptrs, n_frames, widths, heights, format):
    n = len(canvas_ptrs)
    if not (len(n_frames) == len(widths) == len(heights) == n):
        raise ValueError(name + ": the argument lists differ in length")
    if format not in (PNG_RGBA8, PNG_RGBA16):
        raise ValueError(name + ": format is PNG_RGBA8 or PNG_RGBA16")
    px = 8 if format == PNG_RGBA16 else 4
    waves = 0
    for p, f, w, h in zip(canvas_ptrs, n_frames, widths, heights):
        if not p or int(p) % px or int(f) < 1 or not 1 <= int(w) <= 0x7FFFFFFF or not 1 <= int(h) <= 0x7FFFFFFF:
            raise ValueError(name + ": 1 <= width, height <= 2^31 - 1, at least one frame and non-null canvases aligned to a pixel are required")
        groups = -(-int(w) // (16 // px))  # of 16 bytes in a row; a wave takes 64
        waves += int(h) * -(-groups // 64)
    if waves > 0x7FFFFFFF or sum(int(f) for f in n_frames) > 0x7FFFFFFF:
        raise ValueError(name + ": more than 2^31 - 1 canvas rows (counted once per 1024 bytes) or frames in one call")
    return px


def png_diff_batch_device(engine, canvas_ptrs, n_frames, widths, heights, format=PNG_RGBA8, stream=None):
    """The frame diff of many device-resident animations in one call (zs_png_diff_batch_device).  canvas_ptrs[i]: device pointer
    to n_frames[i] canvases of heights[i] * widths[i] * 4 (PNG_RGBA8) or * 8 (PNG_RGBA16) bytes back to back, as
    png_compose_batch_device writes them.  Returns one list per animation of dicts x, y, width, height, dispose_op (0),
    blend_op (0): frame 0 is the whole canvas, frame f >= 1 the smallest rectangle that holds every pixel whose bytes differ
    between canvas f - 1 and canvas f, or 1 x 1 at (0, 0) where none does."""
    name = "png_diff_batch_device"
    _png_canvases_check(name, canvas_ptrs, n_frames, widths, heights, format)
    n = len(canvas_ptrs)
    if n == 0:
        return []
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    fr_arrays = [(_native.PngFrame * int(f))() for f in n_frames]
    rc = _native.lib().zs_png_diff_batch_device(engine.handle, n, VP(*[int(p) for p in canvas_ptrs]), I32(*[int(f) for f in n_frames]),
                                                I64(*[int(x) for x in widths]), I64(*[int(x) for x in heights]), int(format),
                                                (ctypes.POINTER(_native.PngFrame) * n)(*[ctypes.cast(a, ctypes.POINTER(_native.PngFrame)) for a in fr_arrays]),
                                                ctypes.c_void_p(stream or 0))
    if rc != 0:
        raise ValueError("zs_png_diff_batch_device failed (%d): %s" % (rc, engine.last_error()))
    keys = ("x", "y", "width", "height", "dispose_op", "blend_op")
    return [[{k: int(getattr(f, k)) for k in keys} for f in a] for a in fr_arrays]


def png_crop_batch_device(engine, in_ptrs, in_widths, xs, ys, widths, heights, out_ptrs, pixel_bytes=4, stream=None):
    """Rectangles of device-resident images as tight rows in one launch (zs_png_crop_batch_device): the widths[i] x heights[i]
    pixels at (xs[i], ys[i]) of an image whose rows hold in_widths[i] pixels of pixel_bytes (4 or 8) bytes go to out_ptrs[i].
    Pointers are aligned to a pixel and do not overlap; the caller vouches for ys[i] + heights[i]."""
    name = "png_crop_batch_device"
    n = len(in_ptrs)
    if not (len(in_widths) == len(xs) == len(ys) == len(widths) == len(heights) == len(out_ptrs) == n):
        raise ValueError(name + ": the argument lists differ in length")
    if pixel_bytes not in (4, 8):
        raise ValueError(name + ": pixel_bytes is 4 or 8")
    for p, iw, x, y, w, h, o in zip(in_ptrs, in_widths, xs, ys, widths, heights, out_ptrs):
        if not p or not o or int(p) % pixel_bytes or int(o) % pixel_bytes:
            raise ValueError(name + ": non-null device pointers aligned to a pixel are required")
        if not 1 <= int(iw) <= 0x7FFFFFFF or int(w) < 1 or not 1 <= int(h) <= 0x7FFFFFFF or int(x) < 0 or int(y) < 0 or int(x) + int(w) > int(iw) or \
                int(y) + int(h) > 0x7FFFFFFF:
            raise ValueError(name + ": the rectangle lies outside the image's rows")
    if sum(int(h) for h in heights) > 0x7FFFFFFF:
        raise ValueError(name + ": more than 2^31 - 1 rows in one call")
    if n == 0:
        return
    VP, I64 = ctypes.c_void_p * n, ctypes.c_int64 * n
    rc = _native.lib().zs_png_crop_batch_device(engine.handle, n, VP(*[int(p) for p in in_ptrs]), I64(*[int(v) for v in in_widths]), I64(*[int(v) for v in xs]),
                                                I64(*[int(v) for v in ys]), I64(*[int(v) for v in widths]), I64(*[int(v) for v in heights]), int(pixel_bytes),
                                                VP(*[int(p) for p in out_ptrs]), ctypes.c_void_p(stream or 0))
    if rc != 0:
        raise ValueError("zs_png_crop_batch_device failed (%d): %s" % (rc, engine.last_error()))


def png_anim_bound(width, height, n_frames, format=PNG_RGBA8, interlace=0, idat_chunk_bytes=0, extra_len=0):
    """zs_png_anim_bound (host code, no GPU): room that png_encode_anim_batch_device never exceeds for one animation -- every
    frame the whole canvas at 32 or 64 bits a pixel.  -1 for arguments the encoder refuses."""
    args = [int(width), int(height), int(n_frames), int(format), int(interlace), int(idat_chunk_bytes), int(extra_len)]
    if not all(-(1 << 31) <= a < 1 << 31 for a in args[2:5]) or not all(-(1 << 63) <= a < 1 << 63 for a in args):
        return -1
    return int(_native.lib().zs_png_anim_bound(*args))


def png_encode_anim_batch_device(engine, canvas_ptrs, n_frames, widths, heights, filters, out_ptrs, out_caps, delays=None, n_plays=None, format=PNG_RGBA8,
                                 interlace=None, extra=None, rows_per_write=1, idat_chunk_bytes=0, level=6, strategy=0, hash_variant=0, stream=None,
                                 return_status=False):
    """Canvases -> animated PNG files for many device-resident animations in one call (zs_png_encode_anim_batch_device): the
    survey over an animation's canvases, one (colour type, bit depth) pair and one PLTE / tRNS per animation, the frame diff,
    the crop, the pack and the deflate over all frames, then acTL / fcTL / IDAT / fdAT framing.  canvas_ptrs, n_frames, widths,
    heights, format: as for png_diff_batch_device.  delays[i]: n_frames[i] pairs (delay_num, delay_den), each 0 .. 65535
    (None: 1 / 10 for every frame); n_plays[i]: 0 .. 2^31 - 1 (None: 0, for ever).  The rest as for
    png_encode_rgba_batch_device, per animation.  png_anim_bound(...) is always enough room.  One frame gives the still
    encoder's file.  png_decode_anim_batch returns the canvases byte for byte.  Returns (lengths, color_types, bit_depths,
    frames) -- frames[i] one dict per frame, as png_anim_info gives them; return_status: (rc, lengths, statuses, color_types,
    bit_depths, frames)."""
    name = "png_encode_anim_batch_device"
    n = len(canvas_ptrs)
    if interlace is None:
        interlace = [0] * n
    if delays is None:
        delays = [[(1, 10)] * int(f) for f in n_frames]
    if n_plays is None:
        n_plays = [0] * n
    if not (len(filters) == len(out_ptrs) == len(out_caps) == len(interlace) == len(delays) == len(n_plays) == n) or (extra is not None and len(extra) != n):
        raise ValueError(name + ": the argument lists differ in length")
    px = _png_canvases_check(name, canvas_ptrs, n_frames, widths, heights, format)
    if int(rows_per_write) < 0 or not 0 <= int(idat_chunk_bytes) <= 0x7FFFFFFF:
        raise ValueError(name + ": rows_per_write >= 0 and 0 <= idat_chunk_bytes <= 2^31 - 1 are required")
    if not -1 <= int(level) <= 9 or not 0 <= int(strategy) <= 4:
        raise ValueError(name + ": level -1..9 and strategy 0..4 are required")
    total_rows = 0
    for nf, w, h, f, il, o, cap, d, plays in zip(n_frames, widths, heights, filters, interlace, out_ptrs, out_caps, delays, n_plays):
        if not o or not 0 <= int(f) <= 5 or int(cap) < 0 or int(il) not in (0, 1):
            raise ValueError(name + ": filter 0..5, interlace 0 or 1, non-null outputs and non-negative capacities are required")
        if len(d) != int(nf) or any(not 0 <= int(a) <= 65535 or not 0 <= int(b) <= 65535 for a, b in d) or not 0 <= int(plays) <= 0x7FFFFFFF:
            raise ValueError(name + ": one (delay_num, delay_den) pair of values 0 .. 65535 per frame and 0 <= n_plays <= 2^31 - 1 are required")
        if int(nf) * int(h) > 0x7FFFFFFF:
            raise ValueError(name + ": an animation's canvases have more than 2^31 - 1 rows")
        if int(w) * int(h) * px > _CRC_MAX_LEN:
            raise ValueError(name + ": a filtered image is above 2 GiB - 1 KiB")
        total, _, rows = png_idat_layout(w, h, 8 * px, int(il))
        if total > _CRC_MAX_LEN:
            raise ValueError(name + ": a filtered image is above 2 GiB - 1 KiB")
        total_rows += int(nf) * sum(rows)
    if total_rows > 0x7FFFFFFF or sum(int(f) for f in n_frames) > 0x3FFFFFFF:
        raise ValueError(name + ": more than 2^31 - 1 rows or 2^30 - 1 frames in one call")
    if extra is not None:
        extra = [bytes(x) if x is not None else b"" for x in extra]
        if not all(_png_chunks_well_formed(x) for x in extra):
            raise ValueError(name + ": an animation's extra chunks are not a sequence of whole chunks")
    if n == 0:
        return (0, [], [], [], [], []) if return_status else ([], [], [], [])
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    PI32, PFR = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(_native.PngFrame)
    out_len, status, ct, bd = I64(), I32(), I32(), I32()
    num = [(ctypes.c_int * len(d))(*[int(a) for a, _ in d]) for d in delays]
    den = [(ctypes.c_int * len(d))(*[int(b) for _, b in d]) for d in delays]
    fr_arrays = [(_native.PngFrame * int(f))() for f in n_frames]
    x_ptr = VP(*[_host_ptr(x) for x in extra]) if extra is not None else None  # (the bytes objects are read in place: they outlive the call)
    x_len = I64(*[len(x) for x in extra]) if extra is not None else None
    rc = _native.lib().zs_png_encode_anim_batch_device(engine.handle, n, VP(*[int(p) for p in canvas_ptrs]), I32(*[int(f) for f in n_frames]),
                                                       I64(*[int(x) for x in widths]), I64(*[int(x) for x in heights]), int(format),
                                                       (PI32 * n)(*[ctypes.cast(a, PI32) for a in num]), (PI32 * n)(*[ctypes.cast(a, PI32) for a in den]),
                                                       I32(*[int(p) for p in n_plays]), I32(*[int(x) for x in filters]), I32(*[int(x) for x in interlace]),
                                                       x_ptr, x_len, int(rows_per_write), int(idat_chunk_bytes), VP(*[int(p) for p in out_ptrs]),
                                                       I64(*[int(x) for x in out_caps]), out_len, status, (PFR * n)(*[ctypes.cast(a, PFR) for a in fr_arrays]),
                                                       ct, bd, int(level), int(strategy), int(hash_variant), ctypes.c_void_p(stream or 0))
    frames = [[{k: int(getattr(f, k)) for k in _PNG_FRAME_FIELDS} for f in a] for a in fr_arrays]
    if return_status:
        return rc, list(out_len), list(status), list(ct), list(bd), frames
    if rc != 0:
        raise ZlibStreamException("png encode: " + engine.last_error())
    return list(out_len), list(ct), list(bd), frames


WRAP_ZLIB, WRAP_RAW, WRAP_GZIP = 0, 1, 2  # ZS_WRAP_*: RFC 1950, RFC 1951 (no container), RFC 1952


def wrap_bound(n, wrap):
    """zs_wrap_bound (host code): room that deflate_wrap_batch_device needs for n input bytes in container `wrap`."""
    r = _native.lib().zs_wrap_bound(int(n), int(wrap))
    if r < 0:
        raise ValueError("wrap_bound: a negative length or an unknown container")
    return r


def deflate_wrap_batch_device(engine, in_ptrs, in_lens, out_ptrs, out_caps, wrap, level=6, strategy=0, hash_variant=0, stream=None):
    """Device-resident buffers into zlib, raw deflate or gzip streams (zs_deflate_wrap_batch_device; WRAP_ZLIB is
    deflate_batch_device).  Returns (code, lengths, per-stream codes): -5 (ZS_BUF_ERROR) for a stream whose capacity was too
    small -- its length is then what it needs, nothing is written for it and the others are complete."""
    n = len(in_ptrs)
    if not (len(in_lens) == len(out_ptrs) == len(out_caps) == n):
        raise ValueError("deflate_wrap_batch_device: the argument lists differ in length")
    if wrap not in (WRAP_ZLIB, WRAP_RAW, WRAP_GZIP):
        raise ValueError("deflate_wrap_batch_device: an unknown container")
    if n == 0:
        return 0, [], []
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status = I64(), I32()
    rc = _native.lib().zs_deflate_wrap_batch_device(engine.handle, n, VP(*[int(p) for p in in_ptrs]), I64(*[int(x) for x in in_lens]),
                                                    VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), out_len, status,
                                                    int(level), int(strategy), int(hash_variant), int(wrap), ctypes.c_void_p(stream or 0))
    if rc not in (0, -5):
        raise ZlibStreamException("deflating: " + engine.last_error())
    return rc, list(out_len), list(status)


def inflate_wrap_batch_device(engine, in_ptrs, in_lens, out_ptrs, out_caps, wrap, stream=None):
    """Device-resident zlib, raw deflate or gzip streams to bytes (zs_inflate_wrap_batch_device).  Nothing is raised for a
    failing stream: returns (code, output lengths, bytes of input each stream occupies -- 0 for a failing one --, per-stream
    codes: 1 is ZS_STREAM_END); engine.last_error() is the first failing stream's message."""
    n = len(in_ptrs)
    if not (len(in_lens) == len(out_ptrs) == len(out_caps) == n):
        raise ValueError("inflate_wrap_batch_device: the argument lists differ in length")
    if wrap not in (WRAP_ZLIB, WRAP_RAW, WRAP_GZIP):
        raise ValueError("inflate_wrap_batch_device: an unknown container")
    if n == 0:
        return 0, [], [], []
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, in_used, status = I64(), I64(), I32()
    rc = _native.lib().zs_inflate_wrap_batch_device(engine.handle, n, VP(*[int(p) for p in in_ptrs]), I64(*[int(x) for x in in_lens]),
                                                    VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), out_len, in_used,
                                                    status, int(wrap), ctypes.c_void_p(stream or 0))
    if rc == -2:
        raise ValueError("zs_inflate_wrap_batch_device failed: " + engine.last_error())
    return rc, list(out_len), list(in_used), list(status)


_GZIP_INFO_FIELDS = ("bgzf", "xfl", "os", "mtime", "n_members", "name_off", "name_len", "isize_sum")


def gzip_file_info(data):
    """zs_gzip_file_info (host code, no GPU, no engine): a dict of bgzf, xfl, os, mtime, name_off, name_len -- the first
    member's -- and n_members, isize_sum (both -1 unless the file is BGZF).  ZlibStreamException for a file whose first header
    is not gzip's or is cut short, and for a BGZF file whose members' sizes do not walk to its end."""
    data = bytes(data)
    info = _native.GzipInfo()
    rc = _native.lib().zs_gzip_file_info(data, len(data), ctypes.byref(info))
    if rc != 0:
        raise ZlibStreamException("gzip_file_info: not a whole gzip file (%d)" % rc)
    return {k: int(getattr(info, k)) for k in _GZIP_INFO_FIELDS}


def gzip_decode_files_batch(engine, files, out_ptrs, out_caps, stream=None):
    """gzip files (bytes objects in host memory) -> their decoded bytes in device buffers, the members of a file back to
    back, many files a call (zs_gzip_decode_files_batch).  Returns (statuses, lengths, member counts): status 0, or the
    failing member's code (-3 ZS_DATA_ERROR, -5 ZS_BUF_ERROR); engine.last_error() names the first failing file."""
    n = len(files)
    if len(out_ptrs) != n or len(out_caps) != n:
        raise ValueError("gzip_decode_files_batch: the argument lists differ in length")
    if any(not o or int(cap) < 0 for o, cap in zip(out_ptrs, out_caps)):
        raise ValueError("gzip_decode_files_batch: non-null device pointers and non-negative capacities are required")
    if n == 0:
        return [], [], []
    files = [bytes(f) for f in files]
    keep = [ctypes.create_string_buffer(f, len(f)) if f else ctypes.create_string_buffer(1) for f in files]
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, members, status = I64(), I32(), I32()
    rc = _native.lib().zs_gzip_decode_files_batch(engine.handle, n, VP(*[ctypes.addressof(k) for k in keep]), I64(*[len(f) for f in files]),
                                                  VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), out_len, members, status,
                                                  ctypes.c_void_p(stream or 0))
    if rc not in (0, -3, -5):
        raise ValueError("zs_gzip_decode_files_batch failed (%d): %s" % (rc, engine.last_error()))
    return list(status), list(out_len), list(members)


ZIP_AUTO, ZIP_STORED, ZIP_DEFLATED = -1, 0, 8  # ZS_ZIP_*: a zs_zip_put's method
_ZIP_INFO_FIELDS = ("n_entries", "total_len", "cd_off", "cd_len", "shift", "comment_off", "comment_len", "zip64")
_ZIP_ENTRY_FIELDS = ("name_off", "name_len", "method", "flags", "crc32", "comp_len", "len", "local_off", "body_off", "out_off", "dos_time",
                     "dos_date", "external_attr", "status")


def zip_file_info(data):
    """zs_zip_file_info (host code, no GPU, no engine): (info dict, [entry dicts]) of one archive -- the fields of zs_zip_info
    and zs_zip_entry, and per entry "name", the central directory's bytes decoded as UTF-8 where flag bit 11 says so and as
    cp437 otherwise.  An entry the engine cannot decode has a non-zero "status"; ZlibStreamException for a file whose
    directory cannot be walked."""
    data = bytes(data)
    L = _native.lib()
    info = _native.ZipInfo()
    rc = L.zs_zip_file_info(data, len(data), ctypes.byref(info), None, 0)
    if rc != 0:
        raise ZlibStreamException("zip_file_info: not a whole ZIP archive (%d)" % rc)
    n = int(info.n_entries)
    entries = (_native.ZipEntry * max(n, 1))()
    rc = L.zs_zip_file_info(data, len(data), ctypes.byref(info), entries, n)
    if rc != 0:
        raise ZlibStreamException("zip_file_info: not a whole ZIP archive (%d)" % rc)
    out = []
    for e in entries[:n]:
        d = {k: int(getattr(e, k)) for k in _ZIP_ENTRY_FIELDS}
        d["name"] = data[d["name_off"]:d["name_off"] + d["name_len"]].decode("utf-8" if d["flags"] & 0x800 else "cp437")
        out.append(d)
    return {k: int(getattr(info, k)) for k in _ZIP_INFO_FIELDS}, out


def zip_decode_files_batch(engine, files, out_ptrs, out_caps, stream=None):
    """ZIP archives (bytes objects in host memory) -> their entries' bytes in device buffers, entry e of file i at
    out_ptrs[i] + out_off[e] (zip_file_info), many archives a call (zs_zip_decode_files_batch).  Returns (code, lengths,
    per file the list of its entries' codes, per-file codes): a file's code is 0, its own error, or its first failing entry's
    (-3 ZS_DATA_ERROR, -5 ZS_BUF_ERROR); the list of a file whose directory could not be walked, or whose capacity was too
    small, is empty.  engine.last_error() names the first failing file, the entry and the reason."""
    n = len(files)
    if len(out_ptrs) != n or len(out_caps) != n:
        raise ValueError("zip_decode_files_batch: the argument lists differ in length")
    if any(not o or int(cap) < 0 for o, cap in zip(out_ptrs, out_caps)):
        raise ValueError("zip_decode_files_batch: non-null device pointers and non-negative capacities are required")
    if n == 0:
        return 0, [], [], []
    L = _native.lib()
    files = [bytes(f) for f in files]
    keep = [ctypes.create_string_buffer(f, len(f)) if f else ctypes.create_string_buffer(1) for f in files]
    counts = []  # entries whose codes the call writes: none for a file it does not walk or has no room for
    for f, cap in zip(files, out_caps):
        info = _native.ZipInfo()
        walked = len(f) <= _CRC_MAX_LEN and L.zs_zip_file_info(f, len(f), ctypes.byref(info), None, 0) == 0
        counts.append(int(info.n_entries) if walked and info.total_len <= min(int(cap), _CRC_MAX_LEN) else 0)
    per_entry = [(ctypes.c_int * max(k, 1))() for k in counts]
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status = I64(), I32()
    rows = (ctypes.POINTER(ctypes.c_int) * n)(*[ctypes.cast(r, ctypes.POINTER(ctypes.c_int)) for r in per_entry])
    rc = L.zs_zip_decode_files_batch(engine.handle, n, VP(*[ctypes.addressof(k) for k in keep]), I64(*[len(f) for f in files]),
                                     VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), out_len, rows, status,
                                     ctypes.c_void_p(stream or 0))
    if rc not in (0, -3, -5):
        raise ValueError("zs_zip_decode_files_batch failed (%d): %s" % (rc, engine.last_error()))
    return rc, list(out_len), [list(per_entry[i][:counts[i]]) for i in range(n)], list(status)


def _zip_dos(date_time):
    y, mo, d, h, mi, s = date_time
    if not (1980 <= y <= 2107 and 1 <= mo <= 12 and 1 <= d <= 31 and 0 <= h < 24 and 0 <= mi < 60 and 0 <= s < 60):
        raise ValueError("a ZIP entry's date_time must lie in 1980 .. 2107")
    return h << 11 | mi << 5 | s >> 1, (y - 1980) << 9 | mo << 5 | d


def _zip_puts(entries):
    """A list of (name bytes, device ptr, len[, method[, utf8[, date_time[, external_attr]]]]) as a zs_zip_put array; date_time
    is zipfile's (year, month, day, hour, minute, second).  Also returns what keeps the names alive."""
    puts = (_native.ZipPut * max(len(entries), 1))()
    keep = []
    for p, e in zip(puts, entries):
        name, ptr, length = e[0], e[1], e[2]
        method, utf8, date_time, attr = (tuple(e[3:]) + (ZIP_AUTO, 0, (1980, 1, 1, 0, 0, 0), 0)[len(e) - 3:])[:4]
        name = bytes(name)
        keep.append(name)
        p.data, p.len, p.name, p.name_len, p.method, p.utf8 = int(ptr) or None, int(length), name, len(name), int(method), int(bool(utf8))
        p.dos_time, p.dos_date = _zip_dos(date_time)
        p.external_attr = int(attr) & 0xFFFFFFFF
    return puts, keep


def zip_bound(entries):
    """zs_zip_bound (host code): room that zip_encode_batch_device needs for one archive of these entries at the most."""
    puts, keep = _zip_puts(entries)
    r = _native.lib().zs_zip_bound(puts, len(entries))
    if r < 0:
        raise ValueError("zip_bound: more than 65535 entries, a field out of range, or an archive that would need ZIP64")
    return r


def zip_encode_batch_device(engine, archives, out_ptrs, out_caps, level=6, strategy=0, hash_variant=0, stream=None):
    """Device-resident entries into ZIP archives in device buffers, many archives a call (zs_zip_encode_batch_device).
    archives: per archive a list of (name bytes, device ptr, len[, method[, utf8[, date_time[, external_attr]]]]), method
    ZIP_AUTO (the default: deflated unless that is no shorter), ZIP_STORED or ZIP_DEFLATED.  Returns (code, lengths,
    per-archive codes): -5 (ZS_BUF_ERROR) for an archive whose capacity was too small -- its length is then what it needs,
    nothing is written for it and the others are complete."""
    n = len(archives)
    if len(out_ptrs) != n or len(out_caps) != n:
        raise ValueError("zip_encode_batch_device: the argument lists differ in length")
    if n == 0:
        return 0, [], []
    built = [_zip_puts(a) for a in archives]
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status = I64(), I32()
    rows = (ctypes.POINTER(_native.ZipPut) * n)(*[ctypes.cast(p, ctypes.POINTER(_native.ZipPut)) for p, _ in built])
    rc = _native.lib().zs_zip_encode_batch_device(engine.handle if engine is not None else None, n, rows, I32(*[len(a) for a in archives]),
                                                  VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), out_len, status,
                                                  int(level), int(strategy), int(hash_variant), ctypes.c_void_p(stream or 0))
    if rc == -2:
        raise ValueError("zs_zip_encode_batch_device: more than 65535 entries, a field out of range, or an archive that would need ZIP64")
    if rc not in (0, -5):
        raise ZlibStreamException("zip encode: " + engine.last_error())
    return rc, list(out_len), list(status)


_TIFF_INFO_FIELDS = ("n_pages", "big_endian", "bigtiff", "width", "height", "bits", "spp", "sample_format", "photometric", "extra_samples",
                     "extra_kind", "compression", "predictor", "planar", "orientation", "tiled", "chunk_w", "chunk_h", "n_chunks", "row_bytes",
                     "out_len")
_TIFF_CHUNK_FIELDS = ("off", "comp_len", "x", "y", "w", "h", "status")
_TIFF_PUT_DEFAULTS = {"bits": 8, "spp": 1, "sample_format": 1, "photometric": 1, "extra_samples": 0, "extra_kind": 0, "predictor": 1, "tile_width": 0,
                      "tile_height": 0, "rows_per_strip": 0}


def tiff_file_info(data, page=0):
    """zs_tiff_file_info (host code, no GPU, no engine): (info dict, [chunk dicts]) of one page of a TIFF file -- the fields of
    zs_tiff_info and zs_tiff_chunk.  A chunk (a strip or a tile) that the file ends in has a non-zero "status";
    ZlibStreamException, with the library's code in its text, for a file or a page the library does not read."""
    data = bytes(data)
    L = _native.lib()
    info = _native.TiffInfo()
    rc = L.zs_tiff_file_info(data, len(data), int(page), ctypes.byref(info), None, 0)
    if rc != 0:
        raise ZlibStreamException("tiff_file_info: not a TIFF page this library reads (%d)" % rc)
    n = int(info.n_chunks)
    chunks = (_native.TiffChunk * max(n, 1))()
    rc = L.zs_tiff_file_info(data, len(data), int(page), ctypes.byref(info), chunks, n)
    if rc != 0:
        raise ZlibStreamException("tiff_file_info: not a TIFF page this library reads (%d)" % rc)
    return {k: int(getattr(info, k)) for k in _TIFF_INFO_FIELDS}, [{k: int(getattr(c, k)) for k in _TIFF_CHUNK_FIELDS} for c in chunks[:n]]


def tiff_decode_files(engine, files, out_ptrs, out_caps, pages=None, stream=None):
    """TIFF files (bytes objects in host memory) -> the pixels of one page each in device buffers, rows of row_bytes bytes with
    little-endian samples, many files a call (zs_tiff_decode_files_batch).  pages: per file the page, None for page 0 of all.
    Returns (code, lengths, per file the list of its chunks' codes, per-file codes): a file's code is 0, its own error, or its
    first failing chunk's (-3 ZS_DATA_ERROR, -5 ZS_BUF_ERROR); the list of a file whose page could not be walked, or whose
    capacity was too small, is empty.  engine.last_error() names the first failing file, the chunk and the reason."""
    n = len(files)
    if len(out_ptrs) != n or len(out_caps) != n or (pages is not None and len(pages) != n):
        raise ValueError("tiff_decode_files: the argument lists differ in length")
    if any(not o or int(cap) < 0 for o, cap in zip(out_ptrs, out_caps)) or (pages is not None and any(int(p) < 0 for p in pages)):
        raise ValueError("tiff_decode_files: non-null device pointers and non-negative capacities and pages are required")
    if n == 0:
        return 0, [], [], []
    L = _native.lib()
    files = [bytes(f) for f in files]
    keep = [ctypes.create_string_buffer(f, len(f)) if f else ctypes.create_string_buffer(1) for f in files]
    counts = []  # chunks whose codes the call writes: none for a file it does not walk or has no room for
    for i, (f, cap) in enumerate(zip(files, out_caps)):
        info = _native.TiffInfo()
        walked = len(f) <= _CRC_MAX_LEN and L.zs_tiff_file_info(f, len(f), int(pages[i]) if pages is not None else 0, ctypes.byref(info), None, 0) == 0
        counts.append(int(info.n_chunks) if walked and info.out_len <= int(cap) else 0)
    per_chunk = [(ctypes.c_int * max(k, 1))() for k in counts]
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status = I64(), I32()
    rows = (ctypes.POINTER(ctypes.c_int) * n)(*[ctypes.cast(r, ctypes.POINTER(ctypes.c_int)) for r in per_chunk])
    rc = L.zs_tiff_decode_files_batch(engine.handle if engine is not None else None, n, VP(*[ctypes.addressof(k) for k in keep]), I64(*[len(f) for f in files]),
                                      I64(*[int(p) for p in pages]) if pages is not None else None, VP(*[int(p) for p in out_ptrs]),
                                      I64(*[int(x) for x in out_caps]), out_len, rows, status, ctypes.c_void_p(stream or 0))
    if rc not in (0, 2, -3, -5):
        raise ValueError("zs_tiff_decode_files_batch failed (%d): %s" % (rc, engine.last_error() if engine is not None else "no engine"))
    return rc, list(out_len), [list(per_chunk[i][:counts[i]]) for i in range(n)], list(status)


def _tiff_put(image, p=None):
    """A dict of pixels (device pointer), width, height and, where they differ from _TIFF_PUT_DEFAULTS, the other fields of a
    zs_tiff_put."""
    p = p if p is not None else _native.TiffPut()
    unknown = set(image) - set(_TIFF_PUT_DEFAULTS) - {"pixels", "width", "height"}
    if unknown:
        raise ValueError("a TIFF image has no field %s" % sorted(unknown))
    p.pixels, p.width, p.height = int(image["pixels"]) or None, int(image["width"]), int(image["height"])
    for k, v in _TIFF_PUT_DEFAULTS.items():
        setattr(p, k, int(image.get(k, v)))
    return p


def tiff_bound(image):
    """zs_tiff_bound (host code): room that tiff_encode needs for this image (a dict, see tiff_encode) at the most."""
    r = _native.lib().zs_tiff_bound(ctypes.byref(_tiff_put(image)))
    if r < 0:
        raise ValueError("tiff_bound: a field out of range, or a file that would need BigTIFF")
    return r


def tiff_encode(engine, images, out_ptrs, out_caps, level=6, strategy=0, hash_variant=0, stream=None):
    """Device-resident images into Deflate TIFF files in device buffers, many files a call (zs_tiff_encode_batch_device).
    images: per file a dict of pixels (device pointer: height rows of ceil(width * spp * bits / 8) bytes, little-endian), width,
    height and optionally bits (8), spp (1), sample_format (1), photometric (1), extra_samples (0), extra_kind (0), predictor
    (1; 2 horizontal, 3 floating point), tile_width and tile_height (0: strips), rows_per_strip (0: about 256 KiB a strip).
    Returns (code, lengths, per-file codes): -5 (ZS_BUF_ERROR) for a file whose capacity was too small -- its length is then
    what it needs, nothing is written for it and the others are complete."""
    n = len(images)
    if len(out_ptrs) != n or len(out_caps) != n:
        raise ValueError("tiff_encode: the argument lists differ in length")
    if n == 0:
        return 0, [], []
    puts = (_native.TiffPut * n)()
    for p, im in zip(puts, images):
        _tiff_put(im, p)
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status = I64(), I32()
    rc = _native.lib().zs_tiff_encode_batch_device(engine.handle if engine is not None else None, n, puts, VP(*[int(p) for p in out_ptrs]),
                                                   I64(*[int(x) for x in out_caps]), out_len, status, int(level), int(strategy), int(hash_variant),
                                                   ctypes.c_void_p(stream or 0))
    if rc == -2:
        raise ValueError("zs_tiff_encode_batch_device: a field out of range, or a file that would need BigTIFF")
    if rc not in (0, -5):
        raise ZlibStreamException("tiff encode: " + engine.last_error())
    return rc, list(out_len), list(status)


def _tiff_kernel_call(fn, name, engine, in_ptrs, out_ptrs, lists, stream):
    n = len(in_ptrs)
    if len(out_ptrs) != n or any(len(x) != n for x in lists if x is not None):
        raise ValueError(name + ": the argument lists differ in length")
    if n == 0:
        return
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    args = [(I64 if k < 4 else I32)(*[int(v) for v in x]) if x is not None else None for k, x in enumerate(lists)]
    rc = fn(engine.handle if engine is not None else None, n, VP(*[int(p) for p in in_ptrs]), VP(*[int(p) for p in out_ptrs]), *args,
            ctypes.c_void_p(stream or 0))
    if rc == -2:
        raise ValueError(name + ": " + ((engine.last_error() if engine is not None else "") or "stream error"))
    if rc != 0:
        raise ZlibStreamException("%s failed (%d): %s" % (name, rc, engine.last_error()))


def tiff_unpredict(engine, in_ptrs, out_ptrs, widths, heights, bits, spp, predictors, out_widths=None, out_heights=None, big_endian=None, stream=None):
    """Decoded TIFF chunks -> pixels (zs_tiff_unpredict_batch_device, the undo kernel alone): chunk i of widths[i] x heights[i]
    pixels at in_ptrs[i], its top left out_widths[i] x out_heights[i] (default: all of it) to out_ptrs[i], predictor 1, 2 or 3
    undone and big-endian samples swapped.  Device pointers of any alignment."""
    ow, oh = out_widths if out_widths is not None else widths, out_heights if out_heights is not None else heights
    _tiff_kernel_call(_native.lib().zs_tiff_unpredict_batch_device, "tiff_unpredict", engine, in_ptrs, out_ptrs,
                      [widths, heights, ow, oh, bits, spp, predictors, big_endian], stream)


def tiff_predict(engine, in_ptrs, out_ptrs, in_widths, in_heights, bits, spp, predictors, widths=None, heights=None, stream=None):
    """Pixels -> predicted TIFF chunks (zs_tiff_predict_batch_device, the forward kernel alone): in_widths[i] x in_heights[i]
    pixels at in_ptrs[i] into a chunk of widths[i] x heights[i] (default: the same) at out_ptrs[i], the surplus filled by
    repeating the last pixel and row, then differenced (2) or split into byte planes and differenced (3)."""
    w, h = widths if widths is not None else in_widths, heights if heights is not None else in_heights
    _tiff_kernel_call(_native.lib().zs_tiff_predict_batch_device, "tiff_predict", engine, in_ptrs, out_ptrs,
                      [in_widths, in_heights, w, h, bits, spp, predictors], stream)


_EXR_INFO_FIELDS = ("width", "height", "n_channels", "compression", "line_order", "tiled", "has_display_window", "long_names", "tile_w", "tile_h",
                    "lines_per_chunk", "n_chunks", "out_len")
_EXR_CHUNK_FIELDS = ("off", "data_len", "raw_len", "x", "y", "w", "h", "status")
EXR_UINT, EXR_HALF, EXR_FLOAT = 0, 1, 2


def exr_file_info(data):
    """zs_exr_file_info (host code, no GPU, no engine): (info dict, [channel dicts], [chunk dicts]) of an OpenEXR file -- the
    fields of zs_exr_info (the windows as 4-tuples xMin, yMin, xMax, yMax; display_window None where the file has none),
    zs_exr_channel and zs_exr_chunk.  A chunk that the file ends in, or whose header is wrong, has a non-zero "status";
    ZlibStreamException, with the library's code in its text, for a file the library does not read."""
    data = bytes(data)
    L = _native.lib()
    info = _native.ExrInfo()
    rc = L.zs_exr_file_info(data, len(data), ctypes.byref(info), None, 0, None, 0)
    if rc != 0:
        raise ZlibStreamException("exr_file_info: not an OpenEXR file this library reads (%d)" % rc)
    nc, n = int(info.n_channels), int(info.n_chunks)
    channels, chunks = (_native.ExrChannel * max(nc, 1))(), (_native.ExrChunk * max(n, 1))()
    rc = L.zs_exr_file_info(data, len(data), ctypes.byref(info), channels, nc, chunks, n)
    if rc != 0:
        raise ZlibStreamException("exr_file_info: not an OpenEXR file this library reads (%d)" % rc)
    out = {k: int(getattr(info, k)) for k in _EXR_INFO_FIELDS}
    out["data_window"] = tuple(int(v) for v in info.data_window)
    out["display_window"] = tuple(int(v) for v in info.display_window) if info.has_display_window else None
    return (out, [{"name": c.name.decode("latin-1"), "type": int(c.type), "sample_bytes": int(c.sample_bytes), "plane_off": int(c.plane_off)} for c in channels[:nc]],
            [{k: int(getattr(c, k)) for k in _EXR_CHUNK_FIELDS} for c in chunks[:n]])


def exr_decode_files(engine, files, out_ptrs, out_caps, stream=None):
    """OpenEXR files (bytes objects in host memory) -> their channel planes in device buffers (plane c at plane_off[c], H rows
    of W little-endian samples), many files a call (zs_exr_decode_files_batch).  Returns (code, lengths, per file the list of
    its chunks' codes, per-file codes): a file's code is 0, its own error, or its first failing chunk's (-3 ZS_DATA_ERROR,
    -5 ZS_BUF_ERROR); the list of a file whose header could not be walked, or whose capacity was too small, is empty.
    engine.last_error() names the first failing file, the chunk and the reason."""
    n = len(files)
    if len(out_ptrs) != n or len(out_caps) != n:
        raise ValueError("exr_decode_files: the argument lists differ in length")
    if any(not o or int(cap) < 0 for o, cap in zip(out_ptrs, out_caps)):
        raise ValueError("exr_decode_files: non-null device pointers and non-negative capacities are required")
    if n == 0:
        return 0, [], [], []
    L = _native.lib()
    files = [bytes(f) for f in files]
    keep = [ctypes.create_string_buffer(f, len(f)) if f else ctypes.create_string_buffer(1) for f in files]
    counts = []  # chunks whose codes the call writes: none for a file it does not walk or has no room for
    for f, cap in zip(files, out_caps):
        info = _native.ExrInfo()
        walked = len(f) <= _CRC_MAX_LEN and L.zs_exr_file_info(f, len(f), ctypes.byref(info), None, 0, None, 0) == 0
        counts.append(int(info.n_chunks) if walked and info.out_len <= int(cap) else 0)
    per_chunk = [(ctypes.c_int * max(k, 1))() for k in counts]
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status = I64(), I32()
    rows = (ctypes.POINTER(ctypes.c_int) * n)(*[ctypes.cast(r, ctypes.POINTER(ctypes.c_int)) for r in per_chunk])
    rc = L.zs_exr_decode_files_batch(engine.handle if engine is not None else None, n, VP(*[ctypes.addressof(k) for k in keep]), I64(*[len(f) for f in files]),
                                     VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), out_len, rows, status, ctypes.c_void_p(stream or 0))
    if rc not in (0, 2, -3, -5):
        raise ValueError("zs_exr_decode_files_batch failed (%d): %s" % (rc, engine.last_error() if engine is not None else "no engine"))
    return rc, list(out_len), [list(per_chunk[i][:counts[i]]) for i in range(n)], list(status)


def _exr_put(image, p=None):
    """A dict of planes (device pointer), width, height, channels (a list of (name, type) pairs) and optionally x_min, y_min
    (0), compression (3) and extra (bytes) as a zs_exr_put; the arrays it points to hang on the struct."""
    p = p if p is not None else _native.ExrPut()
    unknown = set(image) - {"planes", "width", "height", "channels", "x_min", "y_min", "compression", "extra"}
    if unknown:
        raise ValueError("an OpenEXR image has no field %s" % sorted(unknown))
    channels = list(image["channels"])
    names = [c[0].encode("latin-1") if isinstance(c[0], str) else bytes(c[0]) for c in channels]
    extra = bytes(image.get("extra", b""))
    p._names = (ctypes.c_char_p * max(len(names), 1))(*names)
    p._types = (ctypes.c_int * max(len(names), 1))(*[int(c[1]) for c in channels])
    p._extra = ctypes.create_string_buffer(extra, len(extra)) if extra else None
    p.planes, p.width, p.height = int(image["planes"]) or None, int(image["width"]), int(image["height"])
    p.x_min, p.y_min, p.n_channels, p.compression = int(image.get("x_min", 0)), int(image.get("y_min", 0)), len(names), int(image.get("compression", 3))
    p.names, p.types = p._names, p._types
    p.extra, p.extra_len = ctypes.cast(p._extra, ctypes.c_char_p) if extra else None, len(extra)
    return p


def exr_bound(image):
    """zs_exr_bound (host code): room that exr_encode needs for this image (a dict, see exr_encode) at the most."""
    r = _native.lib().zs_exr_bound(ctypes.byref(_exr_put(image)))
    if r < 0:
        raise ValueError("exr_bound: a field out of range, or channel names that are unsorted, repeated, empty or longer than 31 bytes")
    return r


def exr_encode(engine, images, out_ptrs, out_caps, level=6, strategy=0, hash_variant=0, stream=None):
    """Device-resident channel planes into OpenEXR files in device buffers, many files a call (zs_exr_encode_batch_device).
    images: per file a dict of planes (device pointer: plane c at the running sum of the planes' bytes rounded up to 16, H rows
    of W little-endian samples), width, height, channels (a list of (name, type) pairs sorted byte-wise by name; type 0 UINT,
    1 HALF, 2 FLOAT) and optionally x_min, y_min (0), compression (3 ZIP; 2 ZIPS, 0 none) and extra (encoded attributes).
    Returns (code, lengths, per-file codes): -5 (ZS_BUF_ERROR) for a file whose capacity was too small -- its length is then
    what it needs, nothing is written for it and the others are complete."""
    n = len(images)
    if len(out_ptrs) != n or len(out_caps) != n:
        raise ValueError("exr_encode: the argument lists differ in length")
    if n == 0:
        return 0, [], []
    puts = (_native.ExrPut * n)()
    keep = []  # (an array's element is a copy each time it is read: the arrays of names and types are held here)
    for k, im in enumerate(images):
        q = _exr_put(im)
        keep.append(q)
        ctypes.memmove(ctypes.byref(puts, k * ctypes.sizeof(_native.ExrPut)), ctypes.byref(q), ctypes.sizeof(_native.ExrPut))
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    out_len, status = I64(), I32()
    rc = _native.lib().zs_exr_encode_batch_device(engine.handle if engine is not None else None, n, puts, VP(*[int(p) for p in out_ptrs]),
                                                  I64(*[int(x) for x in out_caps]), out_len, status, int(level), int(strategy), int(hash_variant),
                                                  ctypes.c_void_p(stream or 0))
    if rc == -2:
        raise ValueError("zs_exr_encode_batch_device: a field out of range, or channel names that are unsorted, repeated, empty or longer than 31 bytes")
    if rc not in (0, -5):
        raise ZlibStreamException("exr encode: " + engine.last_error())
    return rc, list(out_len), list(status)


def _exr_kernel_call(fn, name, engine, in_ptrs, out_ptrs, lens, stream):
    n = len(in_ptrs)
    if len(out_ptrs) != n or len(lens) != n:
        raise ValueError(name + ": the argument lists differ in length")
    if n == 0:
        return
    VP, I64 = ctypes.c_void_p * n, ctypes.c_int64 * n
    rc = fn(engine.handle if engine is not None else None, n, VP(*[int(p) for p in in_ptrs]), VP(*[int(p) for p in out_ptrs]), I64(*[int(v) for v in lens]),
            ctypes.c_void_p(stream or 0))
    if rc == -2:
        raise ValueError(name + ": " + ((engine.last_error() if engine is not None else "") or "stream error"))
    if rc != 0:
        raise ZlibStreamException("%s failed (%d): %s" % (name, rc, engine.last_error()))


def exr_unpredict(engine, in_ptrs, out_ptrs, lens, stream=None):
    """Inflated OpenEXR chunks -> their raw bytes (zs_exr_unpredict_batch_device, the undo kernel alone): the running byte sum
    over the whole chunk, then the two halves interleaved.  Device pointers of any alignment, lens[i] in 1 .. 2^31 - 1."""
    _exr_kernel_call(_native.lib().zs_exr_unpredict_batch_device, "exr_unpredict", engine, in_ptrs, out_ptrs, lens, stream)


def exr_predict(engine, in_ptrs, out_ptrs, lens, stream=None):
    """Raw chunk bytes -> what an OpenEXR writer hands to zlib (zs_exr_predict_batch_device, the forward kernel alone)."""
    _exr_kernel_call(_native.lib().zs_exr_predict_batch_device, "exr_predict", engine, in_ptrs, out_ptrs, lens, stream)


CHUNK_STORED, CHUNK_UNSHUFFLED, CHUNK_SKIP, CHUNK_ABSENT = 1, 2, 4, 8  # ZS_CHUNK_*
_GRID_KEYS = {"shape", "chunks", "elem_size", "shuffle", "wrap", "fill", "stored", "level", "dtype"}


def _chunk_grid(grid, g=None):
    """A dict of shape, chunks, elem_size and optionally shuffle (False), wrap (WRAP_ZLIB) and fill (zeros; bytes of one element)
    as a zs_chunk_grid.  The keys stored, level and dtype, which zarr_v2_grid adds, are the caller's to read."""
    g = g if g is not None else _native.ChunkGrid()
    unknown = set(grid) - _GRID_KEYS
    if unknown:
        raise ValueError("a chunk grid has no field %s" % sorted(unknown))
    shape, chunks = [int(v) for v in grid["shape"]], [int(v) for v in grid["chunks"]]
    if len(shape) != len(chunks):
        raise ValueError("a chunk grid's shape and chunks differ in length")
    g.rank, g.elem_size = len(shape), int(grid["elem_size"])
    for d in range(min(len(shape), 8)):
        g.shape[d], g.chunk[d] = shape[d], chunks[d]
    g.shuffle, g.wrap = int(bool(grid.get("shuffle", False))), int(grid.get("wrap", WRAP_ZLIB))
    fill = bytes(grid.get("fill", b"") or b"")
    if fill and len(fill) != g.elem_size:
        raise ValueError("a chunk grid's fill is one element of elem_size bytes")
    for j, b in enumerate(fill[:16]):
        g.fill[j] = b
    return g


def _chunk_grids(grids):
    arr = (_native.ChunkGrid * max(len(grids), 1))()
    for k, grid in enumerate(grids):
        _chunk_grid(grid, arr[k])
    return arr


def chunk_grid_info(grid):
    """zs_chunk_grid_info (host code): (n_chunks, chunk_bytes, array_bytes) of a grid (a dict, see chunks_decode).  ValueError
    for a grid that breaks a rule of include/zsgpu.h: rank 1..8, elem_size 1..16, extents of at least 1, products within int64."""
    n, cb, ab = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    if _native.lib().zs_chunk_grid_info(ctypes.byref(_chunk_grid(grid)), ctypes.byref(n), ctypes.byref(cb), ctypes.byref(ab)) != 0:
        raise ValueError("chunk_grid_info: rank, elem_size, an extent, shuffle or wrap out of range, or a product that leaves int64")
    return n.value, cb.value, ab.value


def chunks_bound(grid):
    """zs_chunks_bound (host code): room that chunks_encode needs for this array at the most."""
    r = _native.lib().zs_chunks_bound(ctypes.byref(_chunk_grid(grid)))
    if r < 0:
        raise ValueError("chunks_bound: a grid out of range")
    return r


FLETCHER32_TILE, DELTA_TILE = 16384, 4096  # ZS_FLETCHER32_TILE (bytes), ZS_DELTA_TILE (elements)
_FILTER_KEYS = ("delta", "byte_order", "fletcher32", "reserved")


def _chunk_filters(filters, n):
    """Per array a dict of delta, byte_order (0 little, 1 big) and fletcher32, each 0 / 1 or a bool and 0 when left out, as
    zs_chunk_filters."""
    if len(filters) != n:
        raise ValueError("the filters and the grids differ in length")
    arr = (_native.ChunkFilters * max(n, 1))()
    for k, f in enumerate(filters):
        unknown = set(f) - set(_FILTER_KEYS)
        if unknown:
            raise ValueError("chunk filters have no field %s" % sorted(unknown))
        for key in _FILTER_KEYS:
            setattr(arr[k], key, int(f.get(key, 0)))
    return arr


def chunks_filters_bound(grid, filters):
    """zs_chunks_filters_bound (host code): chunks_bound(grid) and four more bytes a chunk with fletcher32.  ValueError for a
    grid or a pair of grid and filters out of range (delta or big-endian elements of other than 1, 2, 4 or 8 bytes)."""
    r = _native.lib().zs_chunks_filters_bound(ctypes.byref(_chunk_grid(grid)), _chunk_filters([filters], 1))
    if r < 0:
        raise ValueError("chunks_filters_bound: a grid or its filters out of range")
    return r


def chunks_decode(engine, grids, chunks, out_ptrs, out_caps, stream=None, filters=None):
    """The chunks of HDF5 / NetCDF-4 datasets or Zarr v2 arrays (host bytes) -> the arrays in device buffers, many arrays a call
    (zs_chunks_decode_batch).  grids: per array a dict of shape, chunks, elem_size, shuffle, wrap and fill (zarr_v2_grid makes
    one from a .zarray document).  chunks: per array its n_chunks entries in chunk order (C order over the grid: Zarr's key
    i.j.k) -- bytes, None for a missing chunk (it reads as fill), or a pair (bytes or None, flags) with CHUNK_STORED,
    CHUNK_UNSHUFFLED (HDF5's filter mask) or CHUNK_SKIP (not fetched: the region is left alone); in a grid with stored set every
    chunk is CHUNK_STORED.  Returns (code, per array the list of its chunks' codes, per-array codes): a chunk fails for itself
    only, its region untouched; the list of an array whose capacity was too small (-5) is empty.  engine.last_error() names the
    first failing array, the chunk and the reason.  filters (zs_chunks_decode_filters_batch): per array a dict of delta,
    byte_order and fletcher32 (zarr_v2_filters makes one); a chunk with fletcher32 ends in its four checksum bytes."""
    n = len(grids)
    if len(chunks) != n or len(out_ptrs) != n or len(out_caps) != n:
        raise ValueError("chunks_decode: the argument lists differ in length")
    if n == 0:
        return 0, [], []
    L = _native.lib()
    garr = _chunk_grids(grids)
    keep, refs, counts = [], [], []
    for i, (grid, entries) in enumerate(zip(grids, chunks)):
        n_chunks, _, array_bytes = chunk_grid_info(grid)
        if len(entries) != n_chunks:
            raise ValueError("chunks_decode: array %d has %d chunks, %d were given" % (i, n_chunks, len(entries)))
        r = (_native.ChunkRef * n_chunks)()
        for k, e in enumerate(entries):
            data, flags = e if isinstance(e, tuple) else (e, 0)
            if grid.get("stored"):
                flags |= CHUNK_STORED
            if data is not None:
                data = bytes(data)
                buf = ctypes.create_string_buffer(data, len(data)) if data else ctypes.create_string_buffer(1)
                keep.append(buf)
                r[k].data, r[k].len = ctypes.addressof(buf), len(data)
            r[k].flags = int(flags)
        refs.append(r)
        counts.append(n_chunks if int(out_caps[i]) >= array_bytes else 0)
    per_chunk = [(ctypes.c_int * max(k, 1))() for k in counts]
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    status = I32()
    rows = (ctypes.POINTER(ctypes.c_int) * n)(*[ctypes.cast(r, ctypes.POINTER(ctypes.c_int)) for r in per_chunk])
    ref_rows = (ctypes.POINTER(_native.ChunkRef) * n)(*[ctypes.cast(r, ctypes.POINTER(_native.ChunkRef)) for r in refs])
    args = (ref_rows, VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), rows, status, ctypes.c_void_p(stream or 0))
    if filters is None:
        rc = L.zs_chunks_decode_batch(engine.handle if engine is not None else None, n, garr, *args)
    else:
        rc = L.zs_chunks_decode_filters_batch(engine.handle if engine is not None else None, n, garr, _chunk_filters(filters, n), *args)
    if rc not in (0, 2, -3, -5):
        raise ValueError("zs_chunks_decode_batch failed (%d): %s" % (rc, (engine.last_error() if engine is not None else "") or "stream error"))
    return rc, [list(per_chunk[i][:counts[i]]) for i in range(n)], list(status)


def chunks_encode(engine, grids, in_ptrs, out_ptrs, out_caps, level=6, strategy=0, hash_variant=0, skip_fill=False, allow_stored=False, stream=None, filters=None):
    """Device-resident arrays -> their chunks in device buffers, many arrays a call (zs_chunks_encode_batch_device): shuffled
    where the grid says so, deflated into the grid's container, back to back in chunk order.  skip_fill: a chunk whose existing
    elements all equal fill is not written (CHUNK_ABSENT, length 0).  allow_stored: a chunk whose stream is not shorter than
    its bytes is written as those (CHUNK_STORED), HDF5's rule; without it every chunk is a stream, Zarr's.  Returns (code,
    lengths, per array the list of its chunks' (offset, length, flags), per-array codes): -5 (ZS_BUF_ERROR) for an array whose
    capacity was too small -- its length is then what it needs and nothing is written for it.  filters
    (zs_chunks_encode_filters_batch_device): per array a dict of delta, byte_order and fletcher32; the lengths then include the
    four checksum bytes of a chunk with fletcher32, and chunks_filters_bound is the room."""
    n = len(grids)
    if len(in_ptrs) != n or len(out_ptrs) != n or len(out_caps) != n:
        raise ValueError("chunks_encode: the argument lists differ in length")
    if n == 0:
        return 0, [], [], []
    counts = [chunk_grid_info(g)[0] for g in grids]
    offs, lens, flags = [(ctypes.c_int64 * k)() for k in counts], [(ctypes.c_int64 * k)() for k in counts], [(ctypes.c_int * k)() for k in counts]
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)
    out_len, status = I64(), I32()
    args = (VP(*[int(p) for p in in_ptrs]), VP(*[int(p) for p in out_ptrs]), I64(*[int(x) for x in out_caps]), out_len,
            (P64 * n)(*[ctypes.cast(a, P64) for a in offs]), (P64 * n)(*[ctypes.cast(a, P64) for a in lens]),
            (P32 * n)(*[ctypes.cast(a, P32) for a in flags]), status, int(level), int(strategy), int(hash_variant),
            (1 if skip_fill else 0) | (2 if allow_stored else 0), ctypes.c_void_p(stream or 0))
    if filters is None:
        rc = _native.lib().zs_chunks_encode_batch_device(engine.handle if engine is not None else None, n, _chunk_grids(grids), *args)
    else:
        rc = _native.lib().zs_chunks_encode_filters_batch_device(engine.handle if engine is not None else None, n, _chunk_grids(grids), _chunk_filters(filters, n), *args)
    if rc == -2:
        raise ValueError("zs_chunks_encode_batch_device: " + ((engine.last_error() if engine is not None else "") or "stream error"))
    if rc not in (0, -5):
        raise ZlibStreamException("chunks encode: " + engine.last_error())
    return rc, list(out_len), [list(zip(offs[i], lens[i], flags[i])) for i in range(n)], list(status)


def _shuffle_call(fn, name, engine, in_ptrs, out_ptrs, lens, elem_sizes, stream):
    n = len(in_ptrs)
    if len(out_ptrs) != n or len(lens) != n or len(elem_sizes) != n:
        raise ValueError(name + ": the argument lists differ in length")
    if n == 0:
        return
    VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    rc = fn(engine.handle if engine is not None else None, n, VP(*[int(p) for p in in_ptrs]), VP(*[int(p) for p in out_ptrs]), I64(*[int(v) for v in lens]),
            I32(*[int(v) for v in elem_sizes]), ctypes.c_void_p(stream or 0))
    if rc == -2:
        raise ValueError(name + ": " + ((engine.last_error() if engine is not None else "") or "stream error"))
    if rc != 0:
        raise ZlibStreamException("%s failed (%d): %s" % (name, rc, engine.last_error()))


def shuffle(engine, in_ptrs, out_ptrs, lens, elem_sizes, stream=None):
    """The shuffle filter of HDF5 and numcodecs on device buffers (zs_shuffle_batch_device): byte j of element e to
    j * count + e, count = len // elem_size, the leftover bytes copied behind the planes.  Any alignment, no overlap."""
    _shuffle_call(_native.lib().zs_shuffle_batch_device, "shuffle", engine, in_ptrs, out_ptrs, lens, elem_sizes, stream)


def unshuffle(engine, in_ptrs, out_ptrs, lens, elem_sizes, stream=None):
    """The inverse of shuffle (zs_unshuffle_batch_device)."""
    _shuffle_call(_native.lib().zs_unshuffle_batch_device, "unshuffle", engine, in_ptrs, out_ptrs, lens, elem_sizes, stream)


def fletcher32(engine, ptrs, lens, stream=None):
    """HDF5's Fletcher-32 of device buffers (zs_fletcher32_batch_device): a list of 32-bit checksums.  Any address, lens[i] in
    0 .. 2^31 - 1."""
    n = len(ptrs)
    if len(lens) != n:
        raise ValueError("fletcher32: the argument lists differ in length")
    if n == 0:
        return []
    out = (ctypes.c_uint32 * n)()
    rc = _native.lib().zs_fletcher32_batch_device(engine.handle if engine is not None else None, n, (ctypes.c_void_p * n)(*[int(p) for p in ptrs]),
                                                  (ctypes.c_int64 * n)(*[int(v) for v in lens]), out, ctypes.c_void_p(stream or 0))
    if rc == -2:
        raise ValueError("fletcher32: " + ((engine.last_error() if engine is not None else "") or "stream error"))
    if rc != 0:
        raise ZlibStreamException("fletcher32 failed (%d): %s" % (rc, engine.last_error()))
    return list(out)


def delta_encode(engine, in_ptrs, out_ptrs, lens, elem_sizes, stream=None):
    """numcodecs Delta on device buffers of little-endian elements of 1, 2, 4 or 8 bytes (zs_delta_encode_batch_device):
    out[0] = in[0], out[k] = in[k] - in[k-1], wrapping; the len % elem_size leftover bytes copied.  Any alignment, no overlap."""
    _shuffle_call(_native.lib().zs_delta_encode_batch_device, "delta_encode", engine, in_ptrs, out_ptrs, lens, elem_sizes, stream)


def delta_decode(engine, in_ptrs, out_ptrs, lens, elem_sizes, stream=None):
    """The inverse of delta_encode, a prefix sum (zs_delta_decode_batch_device)."""
    _shuffle_call(_native.lib().zs_delta_decode_batch_device, "delta_decode", engine, in_ptrs, out_ptrs, lens, elem_sizes, stream)


def zarr_v2_filters(zarray_json):
    """A Zarr v2 .zarray document as (grid, filters) for chunks_decode / chunks_encode with filters=.  Beyond zarr_v2_grid it
    accepts big-endian dtypes of 2, 4 and 8 bytes (fill stays in the array's little-endian form) and, in front of the optional
    shuffle, one {"id": "delta", "dtype": D, "astype": D} whose dtype and astype (which may be left out) are the array's dtype, an
    integer of 1, 2, 4 or 8 bytes.  ValueError naming the key for anything else."""
    import json

    import numpy as np
    doc = zarray_json if isinstance(zarray_json, dict) else json.loads(zarray_json.decode() if isinstance(zarray_json, (bytes, bytearray)) else zarray_json)

    def bad(field, why):
        return ValueError("zarr_v2_filters: %s: %s" % (field, why))
    spec, doc = doc.get("dtype"), dict(doc)
    big = False
    if isinstance(spec, str) and len(spec) >= 2 and spec[0] == ">":
        try:
            big = np.dtype(spec).itemsize > 1
        except TypeError:
            raise bad("dtype", "not a dtype numpy knows")
        if big and (np.dtype(spec).itemsize not in (2, 4, 8) or np.dtype(spec).kind in "OUVS"):
            raise bad("dtype", "a big-endian dtype of 2, 4 or 8 bytes is required")
        doc["dtype"] = "<" + spec[1:]
    filters = doc.get("filters") or []
    delta = False
    if isinstance(filters, list) and filters and isinstance(filters[0], dict) and filters[0].get("id") == "delta":
        f = filters[0]
        try:
            dt = np.dtype(spec)
            same = np.dtype(f.get("dtype")) == dt and np.dtype(f.get("astype", f.get("dtype"))) == dt and set(f) <= {"id", "dtype", "astype"}
        except TypeError:
            same = False
        if not isinstance(spec, str) or not same or dt.kind not in "iu" or dt.itemsize not in (1, 2, 4, 8):
            raise bad("filters", "a delta filter whose dtype and astype are the array's integer dtype of 1, 2, 4 or 8 bytes is required")
        delta, doc["filters"] = True, filters[1:]
    try:
        grid = zarr_v2_grid(doc)
    except ValueError as e:
        raise ValueError(str(e).replace("zarr_v2_grid:", "zarr_v2_filters:", 1))
    grid["dtype"] = spec
    return grid, {"delta": int(delta), "byte_order": int(big), "fletcher32": 0}


def zarr_v2_grid(zarray_json):
    """A Zarr v2 .zarray document (str, bytes or the parsed dict) as a grid dict for chunks_decode / chunks_encode.  Pure Python.
    Accepted: zarr_format 2, order "C", a little-endian or single-byte dtype of at most 16 bytes, compressor null, zlib or gzip,
    filters empty or one shuffle whose elementsize is the itemsize; fill_value goes through numpy.  ValueError naming the field
    for anything else.  The dict also has stored (compressor null: every chunk is its plain bytes), level and dtype."""
    import json

    import numpy as np
    doc = zarray_json if isinstance(zarray_json, dict) else json.loads(zarray_json.decode() if isinstance(zarray_json, (bytes, bytearray)) else zarray_json)

    def bad(field, why):
        return ValueError("zarr_v2_grid: %s: %s" % (field, why))
    if doc.get("zarr_format") != 2:
        raise bad("zarr_format", "only 2 is read")
    if doc.get("order") != "C":
        raise bad("order", "only C order is read")
    spec = doc.get("dtype")
    if not isinstance(spec, str) or len(spec) < 2 or spec[0] not in "<|>":
        raise bad("dtype", "a simple dtype string is required")
    try:
        dt = np.dtype(spec)
    except TypeError:
        raise bad("dtype", "not a dtype numpy knows")
    if dt.kind in "OUV" or dt.itemsize < 1 or dt.itemsize > 16 or (spec[0] == ">" and dt.itemsize > 1):
        raise bad("dtype", "a little-endian or single-byte fixed-size dtype of at most 16 bytes is required")
    lists = {}
    for field in ("shape", "chunks"):
        v = doc.get(field)
        if not isinstance(v, list) or not 1 <= len(v) <= 8 or any(not isinstance(x, int) or isinstance(x, bool) or x < 1 for x in v):
            raise bad(field, "1 to 8 extents of at least 1 are required")
        lists[field] = tuple(v)
    if len(lists["shape"]) != len(lists["chunks"]):
        raise bad("chunks", "as many extents as the shape has are required")
    comp = doc.get("compressor")
    if comp is None:
        wrap, level = WRAP_ZLIB, None
    elif isinstance(comp, dict) and comp.get("id") in ("zlib", "gzip"):
        wrap, level = (WRAP_ZLIB if comp["id"] == "zlib" else WRAP_GZIP), comp.get("level")
    else:
        raise bad("compressor", "only null, zlib and gzip are read")
    filters = doc.get("filters") or []
    if not isinstance(filters, list) or len(filters) > 1 or (filters and not (isinstance(filters[0], dict) and filters[0].get("id") == "shuffle" and
                                                                                filters[0].get("elementsize", 4) == dt.itemsize)):
        raise bad("filters", "only one shuffle filter whose elementsize is the itemsize is read")
    fv = doc.get("fill_value")
    try:
        fill = bytes(dt.itemsize) if fv is None else np.array(fv).astype(dt).reshape(()).tobytes()
    except (TypeError, ValueError):
        raise bad("fill_value", "not a value of the dtype")
    return {"shape": lists["shape"], "chunks": lists["chunks"], "elem_size": dt.itemsize, "shuffle": bool(filters), "wrap": wrap, "fill": fill,
            "stored": comp is None, "level": level, "dtype": spec}


_default_engine = None


def default_engine():
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(0)
    return _default_engine


def compress(data, level=6, strategy=0, engine=None):
    """`using (var s = new ZlibOutputStream(ms, level)) s.Write(data)` in one call."""
    return (engine or default_engine()).deflate_batch([data], level, strategy)[0]


class ZlibInputStream(io.RawIOBase):
    """ZlibInputStream.cs: a read-only stream that inflates `base_stream`.

    Same loop as ReadCore (ZlibInputStream.cs:133-186): 8 KiB chunks of BaseStream go to `Inflate(flush)` while the
    caller's buffer has room and the state is ZOK.  The device engine (zs_inflate) takes the chunks in; a whole stream
    is decoded on the GPU at the call that completes it, and a call that arrives without input (BaseStream has nothing more
    for now: a reader behind a writer's flush) decodes the complete blocks of what has arrived and serves them.
    """

    BUFFER_SIZE = 8192

    def __init__(self, base_stream, engine=None):
        super().__init__()
        self.BaseStream = base_stream
        self._engine = engine or default_engine()
        self._lib = _native.lib()
        self._z = self._lib.zs_inflate_init(self._engine.handle, 15)
        if not self._z:
            raise ValueError("zs_inflate_init")
        self._chunk = b""
        self._chunk_pos = 0
        self._no_more_input = False
        self.TotalIn = 0
        self.TotalOut = 0
        self.Adler = 1

    def readable(self):
        return True

    def close(self):
        if getattr(self, "_z", None):
            self._lib.zs_inflate_end(self._z)
            self._z = None
        super().close()

    def __del__(self):
        try:
            if getattr(self, "_z", None):
                self._lib.zs_inflate_end(self._z)
                self._z = None
        except Exception:
            pass

    def readinto(self, b):
        view = memoryview(b).cast("B")
        if len(view) == 0:
            return 0
        out = (ctypes.c_uint8 * len(view))()
        avail_out = ctypes.c_int32(len(view))
        adler, tin, tout = ctypes.c_uint32(self.Adler), ctypes.c_int64(self.TotalIn), ctypes.c_int64(self.TotalOut)
        out_index = 0
        while True:
            if self._chunk_pos == len(self._chunk) and not self._no_more_input:
                self._chunk = self.BaseStream.read(self.BUFFER_SIZE) or b""
                self._chunk_pos = 0
            n_in = len(self._chunk) - self._chunk_pos
            src = (ctypes.c_uint8 * max(1, n_in)).from_buffer_copy(self._chunk[self._chunk_pos:] or b"\0")
            avail_in = ctypes.c_int32(n_in)
            before_out = avail_out.value
            state = self._lib.zs_inflate(self._z, ctypes.cast(src, ctypes.c_void_p), ctypes.byref(avail_in),
                                         ctypes.c_void_p(ctypes.addressof(out) + out_index), ctypes.byref(avail_out), 0,
                                         ctypes.byref(adler), ctypes.byref(tin), ctypes.byref(tout))
            self._chunk_pos += n_in - avail_in.value
            out_index += before_out - avail_out.value
            if state not in (0, 1):
                msg = (self._lib.zs_inflate_message(self._z) or b"").decode()
                raise ZlibStreamException("inflating: " + msg)  # ThrowHelper.cs:21-23
            if not (avail_out.value > 0 and state == 0):
                break
        self.Adler, self.TotalIn, self.TotalOut = adler.value, tin.value, tout.value
        n = len(view) - avail_out.value
        view[:n] = bytes(out)[:n]
        return n


class ZlibOutputStream(io.RawIOBase):
    """ZlibOutputStream.cs: a write-only stream that deflates into `base_stream`.

    Same loop structure as WriteCore / Finish (ZlibOutputStream.cs:125-168,
    213-256): 512-byte chunk buffer, `Deflate(flush)` until the input is
    consumed and the chunk buffer was not filled completely.
    """

    BUFFER_SIZE = 512

    def __init__(self, base_stream, level_or_options=CompressionLevel.DefaultCompression, engine=None, hash_variant=0):
        super().__init__()
        if isinstance(level_or_options, ZlibOptions):
            self.Options = level_or_options
        else:
            self.Options = ZlibOptions(CompressionLevel=level_or_options)
        self.BaseStream = base_stream
        self._engine = engine or default_engine()
        self._lib = _native.lib()
        # ZlibStream.cs:18-29: a null level means inflate mode -- the stream then inflates what is written to it
        self._compress = self.Options.CompressionLevel is not None
        if self._compress:
            level = int(self.Options.CompressionLevel)
            strategy = int(self.Options.CompressionStrategy)
            if level < -1 or level > 9:
                raise ValueError("level")  # ArgumentOutOfRangeException (Deflate.cs:273-276)
            if strategy < 0 or strategy > 4:
                raise ValueError("strategy")
            self._z = self._lib.zs_deflate_init(self._engine.handle, level, strategy, 15, 8, hash_variant)
            if not self._z:
                raise ValueError("zs_deflate_init rejected the arguments")
        else:
            self._z = self._lib.zs_inflate_init(self._engine.handle, 15)
            if not self._z:
                raise ValueError("zs_inflate_init")
        self._chunk = ctypes.create_string_buffer(self.BUFFER_SIZE)
        self._finished = False
        self._total_in = ctypes.c_int64(0)
        self._total_out = ctypes.c_int64(0)
        self._adler = ctypes.c_uint32(1)

    @property
    def TotalIn(self):
        return self._total_in.value

    @property
    def TotalOut(self):
        return self._total_out.value

    def writable(self):
        return True

    def readable(self):
        return False

    def seekable(self):
        return False

    def _deflate_loop(self, data, flush, until_end):
        buf = ctypes.create_string_buffer(bytes(data), len(data)) if len(data) else None
        avail_in = ctypes.c_int32(len(data))
        consumed = 0
        while True:
            avail_out = ctypes.c_int32(self.BUFFER_SIZE)
            next_in = ctypes.c_void_p(ctypes.addressof(buf) + consumed) if buf is not None else ctypes.c_void_p(0)
            before = avail_in.value
            fn = self._lib.zs_deflate if self._compress else self._lib.zs_inflate
            state = fn(self._z, next_in, ctypes.byref(avail_in), ctypes.addressof(self._chunk), ctypes.byref(avail_out), int(flush),
                       ctypes.byref(self._adler), ctypes.byref(self._total_in), ctypes.byref(self._total_out))
            consumed += before - avail_in.value
            if state not in (CompressionState.ZOK, CompressionState.ZSTREAMEND):
                msg = (self._lib.zs_last_message if self._compress else self._lib.zs_inflate_message)(self._z)
                raise ZlibStreamException(("deflating: " if self._compress else "inflating: ") + (msg.decode() if msg else ""))  # ThrowHelper.cs:21-23
            got = self.BUFFER_SIZE - avail_out.value
            if got:
                self.BaseStream.write(self._chunk.raw[:got])
            if not self._compress and avail_in.value == 0 and avail_out.value == 0 and not until_end:
                break  # ZlibOutputStream.cs:155-158
            if state == CompressionState.ZSTREAMEND:
                break
            if not (avail_in.value > 0 or avail_out.value == 0):
                break

    def write(self, b):
        if self._finished:
            raise ValueError("write to finished stream")
        b = bytes(b)
        if len(b) == 0:
            return 0  # WriteCore returns immediately on an empty span
        self._deflate_loop(b, self.Options.FlushMode, False)
        return len(b)

    def WriteByte(self, value):
        self.write(bytes([value]))

    def Finish(self):
        if not self._finished:
            self._deflate_loop(b"", FlushMode.Finish, True)
            self._finished = True
            if hasattr(self.BaseStream, "flush"):
                self.BaseStream.flush()

    def close(self):
        if not self.closed:
            try:
                if getattr(self, "_z", None):
                    self.Finish()
            finally:
                if getattr(self, "_z", None):
                    (self._lib.zs_deflate_end if self._compress else self._lib.zs_inflate_end)(self._z)
                    self._z = None
                super().close()
