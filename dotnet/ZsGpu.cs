// ZsGpu.cs -- P/Invoke surface of libzsgpu.so (include/zsgpu.h), the MI355X deflate / inflate engine.
//
// One declaration per C entry point; the comment on each names the managed code of SixLabors.ZlibStream it stands in
// for.  Nothing here is used by callers directly: ZLibStream.Gpu.cs (the replacement for the internal z_stream
// facade, src/ZlibStream/ZlibStream.cs) is the only consumer, and ZlibOutputStream.cs / ZlibInputStream.cs of the
// reference compile against it unchanged.
using System;
using System.Runtime.InteropServices;

namespace SixLabors.ZlibStream
{
    internal static unsafe class ZsGpu
    {
        // libzsgpu.so next to the assembly or on LD_LIBRARY_PATH (it needs libamdhip64.so from ROCm at run time)
        private const string Lib = "zsgpu";

        // ---- engine context: one per GPU, owns the reusable HBM workspace (no managed counterpart: the managed
        //      engine rents its buffers from ArrayPool, Deflate.Buffers.cs)
        [DllImport(Lib)] public static extern int zs_ctx_create(int device, out IntPtr ctx);
        [DllImport(Lib)] public static extern void zs_ctx_destroy(IntPtr ctx);
        [DllImport(Lib)] public static extern IntPtr zs_ctx_last_error(IntPtr ctx);
        [DllImport(Lib)] public static extern int zs_device_count();
        // counters for tests and diagnostics ("lit_engine_bytes", "fast_rounds", "lit_fallbacks", ...; -1: no such counter)
        [DllImport(Lib)] public static extern long zs_ctx_counter(IntPtr ctx, [MarshalAs(UnmanagedType.LPStr)] string name);

        // ---- Deflate..ctor (Deflate.cs:228-310); IntPtr.Zero where the ctor throws ArgumentOutOfRangeException
        [DllImport(Lib)] public static extern IntPtr zs_deflate_init(IntPtr ctx, int level, int strategy, int windowBits, int memLevel, int hashVariant);

        // ---- Deflate.Compress (Deflate.cs:436-636) as ZLibStream.Deflate(FlushMode) calls it (ZlibStream.cs:164-167)
        [DllImport(Lib)] public static extern int zs_deflate(IntPtr s, byte* nextIn, ref int availIn, byte* nextOut, ref int availOut, int flush,
                                                             ref uint adler, ref long totalIn, ref long totalOut);

        // ---- Deflate.Dispose / ZLibStream.Message
        [DllImport(Lib)] public static extern void zs_deflate_end(IntPtr s);
        [DllImport(Lib)] public static extern IntPtr zs_last_message(IntPtr s);

        // ---- Inflate..ctor (Inflate.cs:76-96), Inflate.Decompress (Inflate.cs:103-357) as ZLibStream.Inflate(FlushMode)
        //      calls it (ZlibStream.cs:119-122), Inflate.Dispose
        [DllImport(Lib)] public static extern IntPtr zs_inflate_init(IntPtr ctx, int windowBits);
        [DllImport(Lib)] public static extern int zs_inflate(IntPtr s, byte* nextIn, ref int availIn, byte* nextOut, ref int availOut, int flush,
                                                             ref uint adler, ref long totalIn, ref long totalOut);
        [DllImport(Lib)] public static extern void zs_inflate_end(IntPtr s);
        [DllImport(Lib)] public static extern IntPtr zs_inflate_message(IntPtr s);

        // ---- throughput entry points for callers that hold many independent buffers (PNG scanline groups, tiles ...):
        //      each buffer is compressed exactly as `using (var s = new ZlibOutputStream(dst, level)) s.Write(buf)` does
        //      (DeflateCorpusBenchmark.cs:86-100); the _multi forms shard the buffers over several contexts / GPUs
        [DllImport(Lib)] public static extern long zs_deflate_bound(long n);
        [DllImport(Lib)] public static extern int zs_deflate_batch(IntPtr ctx, int n, IntPtr* input, long* inLen, IntPtr* output, long* outCap,
                                                                   long* outLen, int* status, int level, int strategy, int hashVariant);
        [DllImport(Lib)] public static extern int zs_inflate_batch(IntPtr ctx, int n, IntPtr* input, long* inLen, IntPtr* output, long* outCap,
                                                                   long* outLen, int* status);
        [DllImport(Lib)] public static extern int zs_deflate_batch_multi(IntPtr* ctxs, int nCtx, int n, IntPtr* input, long* inLen, IntPtr* output,
                                                                         long* outCap, long* outLen, int* status, int level, int strategy, int hashVariant);
        [DllImport(Lib)] public static extern int zs_inflate_batch_multi(IntPtr* ctxs, int nCtx, int n, IntPtr* input, long* inLen, IntPtr* output,
                                                                         long* outCap, long* outLen, int* status);
        // ---- device-resident forms (buffers already in HBM: an encoder whose image lives on the GPU): one stream written in
        //      several NoFlush Writes (writeEnds: the cumulative Write ends, a host array), and the multi-GPU batch over
        //      device pointers (partOf[i]: the context whose GPU holds buffer i, e.g. from zs_partition)
        [DllImport(Lib)] public static extern int zs_partition(long* sizes, int n, int nParts, int* partOf);
        [DllImport(Lib)] public static extern int zs_deflate_writes_device(IntPtr ctx, IntPtr input, long inLen, long* writeEnds, long nWrites, IntPtr output,
                                                                           long outCap, long* outLen, int level, int strategy, int hashVariant, IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_deflate_batch_multi_device(IntPtr* ctxs, int nCtx, int n, IntPtr* input, long* inLen, IntPtr* output,
                                                                                long* outCap, long* outLen, int* status, int* partOf, int level,
                                                                                int strategy, int hashVariant);
        [DllImport(Lib)] public static extern int zs_inflate_batch_multi_device(IntPtr* ctxs, int nCtx, int n, IntPtr* input, long* inLen, IntPtr* output,
                                                                                long* outCap, long* outLen, int* status, int* partOf);
        // ---- the PNG caller path on the device: scanline filtering of an image in HBM (the IDAT payload before compression), and
        //      its inverse over what zs_inflate_batch_device left there (n images, or the Adam7 passes of one, per call)
        [DllImport(Lib)] public static extern int zs_png_filter_device(IntPtr ctx, IntPtr pixels, long rowBytes, long height, int bpp, int filter,
                                                                       IntPtr output, IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_png_unfilter_batch_device(IntPtr ctx, int n, IntPtr* input, long* rowBytes, long* height, int* bpp,
                                                                               IntPtr* output, int* status, IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_png_unfilter_device(IntPtr ctx, IntPtr input, long rowBytes, long height, int bpp, IntPtr output,
                                                                         IntPtr hipStream);
        // ---- the encoder for a batch: n streams each in its own NoFlush Writes (writeEnds[i]: stream i's cumulative ends, or null), the
        //      filter for n images in one launch, and the two together -- pixels in HBM to IDAT payloads in HBM, rowsPerWrite rows a Write.
        //      A stream takes the path it takes alone: scanline Writes at levels 1-3 often mean the one-wave literal engine.
        [DllImport(Lib)] public static extern int zs_deflate_writes_batch_device(IntPtr ctx, int n, IntPtr* input, long* inLen, long** writeEnds, long* nWrites,
                                                                                 IntPtr* output, long* outCap, long* outLen, int* status, int level,
                                                                                 int strategy, int hashVariant, IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_png_filter_batch_device(IntPtr ctx, int n, IntPtr* pixels, long* rowBytes, long* height, int* bpp,
                                                                             int* filter, IntPtr* output, IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_png_idat_batch_device(IntPtr ctx, int n, IntPtr* pixels, long* rowBytes, long* height, int* bpp,
                                                                           int* filter, long rowsPerWrite, IntPtr* output, long* outCap, long* outLen,
                                                                           int* status, int level, int strategy, int hashVariant, IntPtr hipStream);
        // ---- the decoder for a batch: IDAT payloads -> raw scanline pixels in HBM, interlaced (Adam7) or not; the interleave alone; and
        //      the geometry both go by (host code: the inflated size, the seven passes' row bytes and rows)
        [DllImport(Lib)] public static extern int zs_png_decode_batch_device(IntPtr ctx, int n, IntPtr* idat, long* idatLen, long* width, long* height,
                                                                             int* bitsPerPixel, int* interlace, IntPtr* output, int* status,
                                                                             IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_png_adam7_merge_batch_device(IntPtr ctx, int n, IntPtr* passes, long* width, long* height,
                                                                                  int* bitsPerPixel, IntPtr* output, IntPtr hipStream);
        [DllImport(Lib)] public static extern long zs_png_idat_layout(long width, long height, int bitsPerPixel, int interlace, long* rowBytes7,
                                                                      long* rows7);
        // ---- CRC-32 (zlib's crc32) of device-resident bytes, one span or n spans of any lengths in one launch (seed == null: all 0)
        [DllImport(Lib)] public static extern int zs_crc32_device(IntPtr ctx, IntPtr buf, long len, uint seed, uint* crc, IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_crc32_batch_device(IntPtr ctx, int n, IntPtr* buf, long* len, uint* seed, uint* crc, IntPtr hipStream);
        // ---- whole PNG files: pixels in HBM -> files in HBM (signature, IHDR, the caller's chunks from host memory, IDAT chunks of at
        //      most idatChunkBytes data bytes, IEND), the room such a file needs (host code), the chunk walk of one file in host memory
        //      (host code; ancillary chunks are neither verified nor interpreted), and files in host memory -> pixels in HBM
        [DllImport(Lib)] public static extern long zs_png_file_bound(long idatLen, long idatChunkBytes, long extraLen);
        [DllImport(Lib)] public static extern int zs_png_encode_batch_device(IntPtr ctx, int n, IntPtr* pixels, long* width, long* height, int* bitDepth,
                                                                             int* colorType, int* filter, IntPtr* extra, long* extraLen, long rowsPerWrite,
                                                                             long idatChunkBytes, IntPtr* output, long* outCap, long* outLen, int* status,
                                                                             int level, int strategy, int hashVariant, IntPtr hipStream);
        // ---- interlaced encoding (PngEncoder's Adam7 option): the split alone (the inverse of the merge), pixels -> IDAT payloads
        //      and pixels -> files with an interlace value of 0 or 1 per image (interlace == null: all 0)
        [DllImport(Lib)] public static extern int zs_png_adam7_split_batch_device(IntPtr ctx, int n, IntPtr* pixels, long* width, long* height,
                                                                                  int* bitsPerPixel, IntPtr* passesOut, IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_png_idat_interlace_batch_device(IntPtr ctx, int n, IntPtr* pixels, long* width, long* height,
                                                                                     int* bitsPerPixel, int* interlace, int* filter, long rowsPerWrite,
                                                                                     IntPtr* output, long* outCap, long* outLen, int* status, int level,
                                                                                     int strategy, int hashVariant, IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_png_encode_interlace_batch_device(IntPtr ctx, int n, IntPtr* pixels, long* width, long* height,
                                                                                       int* bitDepth, int* colorType, int* filter, int* interlace,
                                                                                       IntPtr* extra, long* extraLen, long rowsPerWrite, long idatChunkBytes,
                                                                                       IntPtr* output, long* outCap, long* outLen, int* status, int level,
                                                                                       int strategy, int hashVariant, IntPtr hipStream);
        [StructLayout(LayoutKind.Sequential)]
        public struct PngInfo
        {
            public long Width, Height;
            public int BitDepth, ColorType, Interlace, BitsPerPixel;
            public long IdatBytes, PixelBytes, IdatChunks;
        }

        [DllImport(Lib)] public static extern int zs_png_file_info(IntPtr file, long len, PngInfo* info);
        [DllImport(Lib)] public static extern int zs_png_decode_files_batch(IntPtr ctx, int n, IntPtr* file, long* fileLen, IntPtr* output, long* outCap,
                                                                            PngInfo* info, int* status, IntPtr hipStream);
        // raw scanlines -> RGBA8 (format 0) or RGBA16 (format 1), PLTE and tRNS applied; the files' colours; files -> RGBA
        [DllImport(Lib)] public static extern int zs_png_expand_batch_device(IntPtr ctx, int n, IntPtr* input, long* width, long* height, int* bitDepth,
                                                                             int* colorType, IntPtr* plte, int* plteEntries, IntPtr* trns, int* trnsLen,
                                                                             int format, IntPtr* output, IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_png_file_colors(IntPtr file, long len, byte* plte768, int* plteEntries, byte* trns256, int* trnsLen);
        [DllImport(Lib)] public static extern int zs_png_decode_files_rgba_batch(IntPtr ctx, int n, IntPtr* file, long* fileLen, int format, IntPtr* output,
                                                                                 long* outCap, PngInfo* info, int* status, IntPtr hipStream);
        // RGBA8 (Rgba32) or RGBA16 (Rgba64) pixels -> raw scanlines of a named pair; what the pixels allow; the pair for that; pixels -> files
        [DllImport(Lib)] public static extern int zs_png_pack_batch_device(IntPtr ctx, int n, IntPtr* input, long* width, long* height, int* bitDepth,
                                                                           int* colorType, IntPtr* plte, int* plteEntries, IntPtr* trns, int* trnsLen,
                                                                           int format, IntPtr* output, long* unmatched, IntPtr hipStream);
        [StructLayout(LayoutKind.Sequential)]
        public struct PngSurvey
        {
            public int Opaque, Gray, Low8, SampleDepth, ColorCount;
            public fixed byte Colors[1024];  // ColorCount x (R, G, B, A), ascending by (A, R, G, B)
        }

        [DllImport(Lib)] public static extern int zs_png_survey_batch_device(IntPtr ctx, int n, IntPtr* input, long* width, long* height, int format,
                                                                             PngSurvey* output, IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_png_choose_format(PngSurvey* survey, int* colorType, int* bitDepth);
        [DllImport(Lib)] public static extern int zs_png_encode_rgba_batch_device(IntPtr ctx, int n, IntPtr* pixels, long* width, long* height, int format,
                                                                                  int* filter, int* interlace, IntPtr* extra, long* extraLen,
                                                                                  long rowsPerWrite, long idatChunkBytes, IntPtr* output, long* outCap,
                                                                                  long* outLen, int* status, int* colorTypeOut, int* bitDepthOut, int level,
                                                                                  int strategy, int hashVariant, IntPtr hipStream);
        // animated PNG: the frames of a file (host code); frames -> canvases on the device; files -> composed canvases
        [StructLayout(LayoutKind.Sequential)]
        public struct PngFrame
        {
            public long X, Y, Width, Height;
            public int DelayNum, DelayDen;
            public int DisposeOp, BlendOp;  // 0 NONE, 1 BACKGROUND, 2 PREVIOUS; 0 SOURCE, 1 OVER
            public long DataBytes, DataChunks;
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct PngAnim
        {
            public PngInfo Png;
            public int Animated, FrameCount, PlayCount, DefaultIsFrame;
        }

        [DllImport(Lib)] public static extern int zs_png_anim_info(IntPtr file, long len, PngAnim* anim, PngFrame* frames, int framesCap);
        [DllImport(Lib)] public static extern int zs_png_compose_batch_device(IntPtr ctx, int n, IntPtr** framePixels, PngFrame** frames, int* frameCount,
                                                                              long* width, long* height, int format, IntPtr* output, IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_png_decode_anim_batch(IntPtr ctx, int n, IntPtr* file, long* fileLen, int format, IntPtr* output,
                                                                           long* outCap, PngAnim* anim, int* status, IntPtr hipStream);
        // animated PNG on the way out: canvases -> the frames' regions; rectangles -> tight rows; canvases -> files
        [DllImport(Lib)] public static extern int zs_png_diff_batch_device(IntPtr ctx, int n, IntPtr* canvases, int* frameCount, long* width, long* height,
                                                                           int format, PngFrame** framesOut, IntPtr hipStream);
        [DllImport(Lib)] public static extern int zs_png_crop_batch_device(IntPtr ctx, int n, IntPtr* input, long* inWidth, long* x, long* y, long* width,
                                                                           long* height, int pixelBytes, IntPtr* output, IntPtr hipStream);
        [DllImport(Lib)] public static extern long zs_png_anim_bound(long width, long height, int frameCount, int format, int interlace, long idatChunkBytes,
                                                                     long extraLen);
        [DllImport(Lib)] public static extern int zs_png_encode_anim_batch_device(IntPtr ctx, int n, IntPtr* canvases, int* frameCount, long* width, long* height,
                                                                                  int format, int** delayNum, int** delayDen, int* playCount, int* filter,
                                                                                  int* interlace, IntPtr* extra, long* extraLen, long rowsPerWrite,
                                                                                  long idatChunkBytes, IntPtr* output, long* outCap, long* outLen, int* status,
                                                                                  PngFrame** framesOut, int* colorTypeOut, int* bitDepthOut, int level,
                                                                                  int strategy, int hashVariant, IntPtr hipStream);
        // bytes fed behind a stream's trailer before its end was seen (the engine looks for the end now and then)
        [DllImport(Lib)] public static extern long zs_inflate_surplus(IntPtr s, IntPtr* p);
    }

    /// <summary>
    /// The process-wide engine context of one GPU.  A zs_ctx is not thread-safe (like a managed Deflate instance), so
    /// calls into it are serialised by <see cref="Gate"/>; streams on different GPUs use different contexts.
    /// </summary>
    internal sealed class GpuContext : IDisposable
    {
        private static readonly object InitLock = new object();
        private static GpuContext shared;

        private GpuContext(int device)
        {
            int rc = ZsGpu.zs_ctx_create(device, out IntPtr h);
            if (rc != 0 || h == IntPtr.Zero)
            {
                // there is deliberately no managed fallback: a silent CPU path would hide a mis-deployed library
                throw new ZlibStreamException("no usable MI355X / HIP device (zs_ctx_create returned " + rc + ")");
            }

            this.Handle = h;
        }

        public IntPtr Handle { get; private set; }

        public object Gate { get; } = new object();

        public static GpuContext Shared
        {
            get
            {
                lock (InitLock)
                {
                    if (shared is null)
                    {
                        string dev = Environment.GetEnvironmentVariable("ZSGPU_DEVICE");
                        shared = new GpuContext(string.IsNullOrEmpty(dev) ? 0 : int.Parse(dev));
                    }

                    return shared;
                }
            }
        }

        public void Dispose()
        {
            if (this.Handle != IntPtr.Zero)
            {
                ZsGpu.zs_ctx_destroy(this.Handle);
                this.Handle = IntPtr.Zero;
            }
        }
    }
}
