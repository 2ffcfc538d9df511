// zsgpu.hpp -- C++ host-side mirror of the reference's Stream API over the C ABI (zsgpu.h).
//
// The reference is compiled managed code (C#) and no .NET toolchain exists in the build image, so the host
// side above the C ABI is written in C++: same type names, members, argument meaning and error behaviour as
//   src/ZlibStream/ZlibOutputStream.cs, ZlibInputStream.cs, ZlibOptions.cs, CompressionLevel.cs,
//   CompressionStrategy.cs, FlushMode.cs, CompressionState.cs, ZlibStreamException.cs, ThrowHelper.cs:21-23,
// with System.IO.Stream replaced by std::ostream / std::istream.  Header-only; link with libzsgpu.so.
#pragma once
#include <cstdint>
#include <istream>
#include <optional>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "zsgpu.h"

namespace SixLabors {
namespace ZlibStream {

enum class CompressionLevel : int {  // CompressionLevel.cs
    DefaultCompression = -1, Level0 = 0, NoCompression = 0, Level1 = 1, BestSpeed = 1, Level2 = 2, Level3 = 3, Level4 = 4,
    Level5 = 5, Level6 = 6, Level7 = 7, Level8 = 8, Level9 = 9, BestCompression = 9
};
enum class CompressionStrategy : int { DefaultStrategy = 0, Filtered = 1, HuffmanOnly = 2, Rle = 3, Fixed = 4 };
enum class FlushMode : int { NoFlush = 0, PartialFlush = 1, SyncFlush = 2, FullFlush = 3, Finish = 4 };
enum class CompressionState : int {
    ZVERSIONERROR = -6, ZBUFERROR = -5, ZMEMERROR = -4, ZDATAERROR = -3, ZSTREAMERROR = -2, ZERRNO = -1, ZOK = 0, ZSTREAMEND = 1,
    ZNEEDDICT = 2
};

struct ZlibOptions {  // ZlibOptions.cs
    std::optional<CompressionLevel> CompressionLevel_;
    CompressionStrategy CompressionStrategy_ = CompressionStrategy::DefaultStrategy;
    FlushMode FlushMode_ = FlushMode::NoFlush;
};

class ZlibStreamException : public std::runtime_error {  // ZlibStreamException.cs
public:
    explicit ZlibStreamException(const std::string &m) : std::runtime_error(m) {}
};

// One engine context per GPU, shared by the streams of the process (zs_ctx is not thread-safe).
class GpuContext {
public:
    static zs_ctx *Shared(int device = 0) {
        static GpuContext g(device);
        return g.ctx_;
    }
private:
    explicit GpuContext(int device) {
        if (zs_ctx_create(device, &ctx_) != ZS_OK || !ctx_)
            throw ZlibStreamException("no usable MI355X / HIP device: the engine has no CPU fallback");
    }
    ~GpuContext() { zs_ctx_destroy(ctx_); }
    zs_ctx *ctx_ = nullptr;
};

// The decode half of the PNG caller path for an image that stays on the GPU: what zs_inflate_batch_device left for an IDAT
// payload (device pointer, height rows of 1 + rowBytes bytes) -> height * rowBytes bytes of pixels (device pointer).
inline void PngUnfilterDevice(const void *filtered, int64_t rowBytes, int64_t height, int bytesPerPixel, void *pixels, zs_ctx *ctx = nullptr,
                              void *hipStream = nullptr) {
    zs_ctx *c = ctx ? ctx : GpuContext::Shared();
    const int rc = zs_png_unfilter_device(c, filtered, rowBytes, height, bytesPerPixel, pixels, hipStream);
    if (rc != ZS_OK) throw ZlibStreamException(rc == ZS_DATA_ERROR ? std::string("png: ") + zs_ctx_last_error(c) : std::string("png: bad arguments"));
}

// The whole decode path for images that stay on the GPU, n a call: idat[i] (device pointer, idatLen[i] bytes: the image's IDAT
// data concatenated, one zlib stream) -> pixels[i] (device pointer, height[i] rows of ceil(width[i] * bitsPerPixel[i] / 8)
// bytes of raw scanline data), interlaced (Adam7) or not.  Returns a status per image: ZS_OK, or ZS_DATA_ERROR for an image
// that does not decode (zs_ctx_last_error names the first one; the others are complete).
inline std::vector<int> PngDecodeBatchDevice(const std::vector<const void *> &idat, const std::vector<int64_t> &idatLen, const std::vector<int64_t> &width,
                                             const std::vector<int64_t> &height, const std::vector<int> &bitsPerPixel, const std::vector<int> &interlace,
                                             const std::vector<void *> &pixels, zs_ctx *ctx = nullptr, void *hipStream = nullptr) {
    const size_t n = idat.size();
    if (idatLen.size() != n || width.size() != n || height.size() != n || bitsPerPixel.size() != n || interlace.size() != n || pixels.size() != n)
        throw ZlibStreamException("png: the argument lists differ in length");
    zs_ctx *c = ctx ? ctx : GpuContext::Shared();
    std::vector<int> status(n, 0);
    const int rc = zs_png_decode_batch_device(c, (int)n, idat.data(), idatLen.data(), width.data(), height.data(), bitsPerPixel.data(), interlace.data(),
                                              pixels.data(), status.data(), hipStream);
    if (rc != ZS_OK && rc != ZS_DATA_ERROR) throw ZlibStreamException(rc == ZS_MEM_ERROR ? std::string("png: out of device memory") : std::string("png: bad arguments"));
    return status;
}
// ... its last step alone, for a caller that reconstructs the passes itself: passes[i] (device pointer, the seven passes back
// to back without filter bytes, absent ones absent; zs_png_idat_layout gives their sizes) -> pixels[i]
inline void PngAdam7MergeBatchDevice(const std::vector<const void *> &passes, const std::vector<int64_t> &width, const std::vector<int64_t> &height,
                                     const std::vector<int> &bitsPerPixel, const std::vector<void *> &pixels, zs_ctx *ctx = nullptr,
                                     void *hipStream = nullptr) {
    const size_t n = passes.size();
    if (width.size() != n || height.size() != n || bitsPerPixel.size() != n || pixels.size() != n)
        throw ZlibStreamException("png: the argument lists differ in length");
    zs_ctx *c = ctx ? ctx : GpuContext::Shared();
    if (zs_png_adam7_merge_batch_device(c, (int)n, passes.data(), width.data(), height.data(), bitsPerPixel.data(), pixels.data(), hipStream) != ZS_OK)
        throw ZlibStreamException("png: bad arguments");
}
// ... and the geometry both go by (host code): the inflated size of an image's IDAT payload, -1 for bad arguments
inline int64_t PngIdatLayout(int64_t width, int64_t height, int bitsPerPixel, bool interlace, int64_t rowBytes[7] = nullptr, int64_t rows[7] = nullptr) {
    return zs_png_idat_layout(width, height, bitsPerPixel, interlace ? 1 : 0, rowBytes, rows);
}

// zlib's crc32 of device-resident spans of any lengths and alignments, n a launch (zs_crc32_batch_device); seed: empty (all 0)
// or one per span -- a result fed back as the seed continues a CRC.
inline std::vector<uint32_t> Crc32BatchDevice(const std::vector<const void *> &buf, const std::vector<int64_t> &len, const std::vector<uint32_t> &seed = {},
                                              zs_ctx *ctx = nullptr, void *hipStream = nullptr) {
    const size_t n = buf.size();
    if (len.size() != n || (!seed.empty() && seed.size() != n)) throw ZlibStreamException("crc32: the argument lists differ in length");
    zs_ctx *c = ctx ? ctx : GpuContext::Shared();
    std::vector<uint32_t> crc(n, 0);
    const int rc = zs_crc32_batch_device(c, (int)n, buf.data(), len.data(), seed.empty() ? nullptr : seed.data(), crc.data(), hipStream);
    if (rc != ZS_OK) throw ZlibStreamException(rc == ZS_MEM_ERROR ? std::string("crc32: out of device memory") : std::string("crc32: bad arguments"));
    return crc;
}
inline uint32_t Crc32Device(const void *buf, int64_t len, uint32_t seed = 0, zs_ctx *ctx = nullptr, void *hipStream = nullptr) {
    uint32_t crc = 0;
    if (zs_crc32_device(ctx ? ctx : GpuContext::Shared(), buf, len, seed, &crc, hipStream) != ZS_OK) throw ZlibStreamException("crc32: bad arguments");
    return crc;
}

// Whole PNG files.  Room for the file around a zlib stream of idatLen bytes (host code; -1 for bad arguments) ...
inline int64_t PngFileBound(int64_t idatLen, int64_t idatChunkBytes = 0, int64_t extraLen = 0) { return zs_png_file_bound(idatLen, idatChunkBytes, extraLen); }
namespace detail {
// the one body of PngEncodeBatchDevice and PngEncodeInterlaceBatchDevice: the length checks, the extra chunks' pointers and the
// error mapping.  interlace null: zs_png_encode_batch_device; else zs_png_encode_interlace_batch_device (an empty list: all 0)
inline std::vector<int64_t> PngEncodeFiles(const std::vector<const void *> &pixels, const std::vector<int64_t> &width, const std::vector<int64_t> &height,
                                           const std::vector<int> &bitDepth, const std::vector<int> &colorType, const std::vector<int> &filter,
                                           const std::vector<int> *interlace, const std::vector<std::string> &extra, int64_t rowsPerWrite, int64_t idatChunkBytes,
                                           const std::vector<void *> &out, const std::vector<int64_t> &outCap, std::vector<int> *status, int level, int strategy,
                                           zs_ctx *ctx, void *hipStream) {
    const size_t n = pixels.size();
    if (width.size() != n || height.size() != n || bitDepth.size() != n || colorType.size() != n || filter.size() != n || out.size() != n || outCap.size() != n ||
        (!extra.empty() && extra.size() != n) || (interlace && !interlace->empty() && interlace->size() != n))
        throw ZlibStreamException("png: the argument lists differ in length");
    zs_ctx *c = ctx ? ctx : GpuContext::Shared();
    std::vector<const void *> xp(n, nullptr);
    std::vector<int64_t> xl(n, 0), outLen(n, 0);
    for (size_t i = 0; i < extra.size(); i++) xp[i] = extra[i].data(), xl[i] = (int64_t)extra[i].size();
    std::vector<int> st(n, 0);
    const void *const *xpp = extra.empty() ? nullptr : xp.data();
    const int64_t *xlp = extra.empty() ? nullptr : xl.data();
    const int rc = interlace ? zs_png_encode_interlace_batch_device(c, (int)n, pixels.data(), width.data(), height.data(), bitDepth.data(), colorType.data(),
                                                                    filter.data(), interlace->empty() ? nullptr : interlace->data(), xpp, xlp, rowsPerWrite,
                                                                    idatChunkBytes, out.data(), outCap.data(), outLen.data(), st.data(), level, strategy, 0, hipStream)
                             : zs_png_encode_batch_device(c, (int)n, pixels.data(), width.data(), height.data(), bitDepth.data(), colorType.data(), filter.data(), xpp,
                                                          xlp, rowsPerWrite, idatChunkBytes, out.data(), outCap.data(), outLen.data(), st.data(), level, strategy, 0,
                                                          hipStream);
    if (status) *status = st;
    if (rc != ZS_OK && !(rc == ZS_BUF_ERROR && status)) throw ZlibStreamException(std::string("png encode: ") + zs_ctx_last_error(c));
    return outLen;
}
}  // namespace detail
// ... pixels on the GPU -> complete files on the GPU, n a call: pixels[i] (device pointer, height[i] rows of raw scanline data)
// -> out[i] (device pointer, outCap[i] bytes): signature, IHDR, extra[i] (chunks the caller has framed, host bytes, verbatim; the
// list may be empty), the stream of PngIdatBatchDevice in IDAT chunks of at most idatChunkBytes data bytes (0: one chunk), IEND.
// Returns the files' lengths; status (optional) receives ZS_OK or ZS_BUF_ERROR per image.
inline std::vector<int64_t> PngEncodeBatchDevice(const std::vector<const void *> &pixels, const std::vector<int64_t> &width, const std::vector<int64_t> &height,
                                                 const std::vector<int> &bitDepth, const std::vector<int> &colorType, const std::vector<int> &filter,
                                                 const std::vector<std::string> &extra, int64_t rowsPerWrite, int64_t idatChunkBytes,
                                                 const std::vector<void *> &out, const std::vector<int64_t> &outCap, std::vector<int> *status = nullptr,
                                                 CompressionLevel level = CompressionLevel::DefaultCompression,
                                                 CompressionStrategy strategy = CompressionStrategy::DefaultStrategy, zs_ctx *ctx = nullptr,
                                                 void *hipStream = nullptr) {
    return detail::PngEncodeFiles(pixels, width, height, bitDepth, colorType, filter, nullptr, extra, rowsPerWrite, idatChunkBytes, out, outCap, status, (int)level,
                                  (int)strategy, ctx, hipStream);
}
// ... the same with IHDR's interlace byte per image (zs_png_encode_interlace_batch_device; interlace empty: all 0, and the files
// are PngEncodeBatchDevice's): an image with interlace 1 is split into its Adam7 passes on the device, every pass filtered on
// its own, rowsPerWrite counting pass rows ...
inline std::vector<int64_t> PngEncodeInterlaceBatchDevice(const std::vector<const void *> &pixels, const std::vector<int64_t> &width,
                                                          const std::vector<int64_t> &height, const std::vector<int> &bitDepth, const std::vector<int> &colorType,
                                                          const std::vector<int> &filter, const std::vector<int> &interlace, const std::vector<std::string> &extra,
                                                          int64_t rowsPerWrite, int64_t idatChunkBytes, const std::vector<void *> &out,
                                                          const std::vector<int64_t> &outCap, std::vector<int> *status = nullptr,
                                                          CompressionLevel level = CompressionLevel::DefaultCompression,
                                                          CompressionStrategy strategy = CompressionStrategy::DefaultStrategy, zs_ctx *ctx = nullptr,
                                                          void *hipStream = nullptr) {
    return detail::PngEncodeFiles(pixels, width, height, bitDepth, colorType, filter, &interlace, extra, rowsPerWrite, idatChunkBytes, out, outCap, status, (int)level,
                                  (int)strategy, ctx, hipStream);
}
// ... its first half, pixels -> the IDAT payloads' zlib streams (zs_png_idat_interlace_batch_device; interlace empty: all 0) ...
inline std::vector<int64_t> PngIdatInterlaceBatchDevice(const std::vector<const void *> &pixels, const std::vector<int64_t> &width,
                                                        const std::vector<int64_t> &height, const std::vector<int> &bitsPerPixel, const std::vector<int> &interlace,
                                                        const std::vector<int> &filter, int64_t rowsPerWrite, const std::vector<void *> &out,
                                                        const std::vector<int64_t> &outCap, CompressionLevel level = CompressionLevel::DefaultCompression,
                                                        CompressionStrategy strategy = CompressionStrategy::DefaultStrategy, zs_ctx *ctx = nullptr,
                                                        void *hipStream = nullptr) {
    const size_t n = pixels.size();
    if (width.size() != n || height.size() != n || bitsPerPixel.size() != n || filter.size() != n || out.size() != n || outCap.size() != n ||
        (!interlace.empty() && interlace.size() != n))
        throw ZlibStreamException("png: the argument lists differ in length");
    zs_ctx *c = ctx ? ctx : GpuContext::Shared();
    std::vector<int64_t> outLen(n, 0);
    std::vector<int> st(n, 0);
    if (zs_png_idat_interlace_batch_device(c, (int)n, pixels.data(), width.data(), height.data(), bitsPerPixel.data(), interlace.empty() ? nullptr : interlace.data(),
                                           filter.data(), rowsPerWrite, out.data(), outCap.data(), outLen.data(), st.data(), (int)level, (int)strategy, 0,
                                           hipStream) != ZS_OK)
        throw ZlibStreamException(std::string("png idat: ") + zs_ctx_last_error(c));
    return outLen;
}
// ... and the split alone, the inverse of PngAdam7MergeBatchDevice: pixels[i] -> passes[i] (device pointers; the present passes
// back to back without filter bytes, PngIdatLayout's size minus one byte per pass row)
inline void PngAdam7SplitBatchDevice(const std::vector<const void *> &pixels, const std::vector<int64_t> &width, const std::vector<int64_t> &height,
                                     const std::vector<int> &bitsPerPixel, const std::vector<void *> &passes, zs_ctx *ctx = nullptr,
                                     void *hipStream = nullptr) {
    const size_t n = pixels.size();
    if (width.size() != n || height.size() != n || bitsPerPixel.size() != n || passes.size() != n)
        throw ZlibStreamException("png: the argument lists differ in length");
    zs_ctx *c = ctx ? ctx : GpuContext::Shared();
    if (zs_png_adam7_split_batch_device(c, (int)n, pixels.data(), width.data(), height.data(), bitsPerPixel.data(), passes.data(), hipStream) != ZS_OK)
        throw ZlibStreamException(std::string("png split: ") + zs_ctx_last_error(c));
}
// ... the chunk walk of one file in host memory (host code; throws for a file that is not a whole PNG) ...
inline zs_png_info PngFileInfo(const void *file, int64_t len) {
    zs_png_info info{};
    if (zs_png_file_info(file, len, &info) != ZS_OK) throw ZlibStreamException("png: not a whole PNG file");
    return info;
}
// ... and files in host memory -> pixels on the GPU, n a call (zs_png_decode_files_batch): returns a status per file (ZS_OK,
// ZS_BUF_ERROR, ZS_DATA_ERROR -- zs_ctx_last_error names the first failing file and the reason), info (optional) what each says.
inline std::vector<int> PngDecodeFilesBatch(const std::vector<const void *> &file, const std::vector<int64_t> &fileLen, const std::vector<void *> &pixels,
                                            const std::vector<int64_t> &pixelsCap, std::vector<zs_png_info> *info = nullptr, zs_ctx *ctx = nullptr,
                                            void *hipStream = nullptr) {
    const size_t n = file.size();
    if (fileLen.size() != n || pixels.size() != n || pixelsCap.size() != n) throw ZlibStreamException("png: the argument lists differ in length");
    zs_ctx *c = ctx ? ctx : GpuContext::Shared();
    std::vector<int> status(n, 0);
    if (info) info->assign(n, zs_png_info{});
    const int rc = zs_png_decode_files_batch(c, (int)n, file.data(), fileLen.data(), pixels.data(), pixelsCap.data(), info ? info->data() : nullptr, status.data(),
                                             hipStream);
    if (rc != ZS_OK && rc != ZS_DATA_ERROR && rc != ZS_BUF_ERROR)
        throw ZlibStreamException(rc == ZS_MEM_ERROR ? std::string("png: out of device memory") : std::string("png: bad arguments"));
    return status;
}

// The encode half for images that stay on the GPU, n a call: pixels[i] (device pointer, height[i] rows of rowBytes[i] bytes)
// -> the zlib stream of image i's IDAT payload in out[i] (device pointer, outCap[i] bytes), rows filtered with filter[i]
// (0-4, 5 adaptive) and written rowsPerWrite rows a Write, as a scanline encoder writes to ZlibOutputStream (1; 0: one Write
// per image).  Returns the streams' lengths.  (The two halves follow.
// At levels 1-3 scanline Writes often put a stream on the one-wave literal engine, as they do one image at a time.)
inline std::vector<int64_t> PngIdatBatchDevice(const std::vector<const void *> &pixels, const std::vector<int64_t> &rowBytes,
                                               const std::vector<int64_t> &height, const std::vector<int> &bytesPerPixel, const std::vector<int> &filter,
                                               int64_t rowsPerWrite, const std::vector<void *> &out, const std::vector<int64_t> &outCap,
                                               CompressionLevel level = CompressionLevel::DefaultCompression,
                                               CompressionStrategy strategy = CompressionStrategy::DefaultStrategy, zs_ctx *ctx = nullptr,
                                               void *hipStream = nullptr) {
    const size_t n = pixels.size();
    if (rowBytes.size() != n || height.size() != n || bytesPerPixel.size() != n || filter.size() != n || out.size() != n || outCap.size() != n)
        throw ZlibStreamException("png: the argument lists differ in length");
    zs_ctx *c = ctx ? ctx : GpuContext::Shared();
    std::vector<int64_t> outLen(n, 0);
    std::vector<int> status(n, 0);
    const int rc = zs_png_idat_batch_device(c, (int)n, pixels.data(), rowBytes.data(), height.data(), bytesPerPixel.data(), filter.data(), rowsPerWrite,
                                            out.data(), outCap.data(), outLen.data(), status.data(), (int)level, (int)strategy, 0, hipStream);
    if (rc != ZS_OK) throw ZlibStreamException(std::string("deflating: ") + zs_ctx_last_error(c));
    return outLen;
}

// The two halves of PngIdatBatchDevice for a caller that wants the filtered rows, or has them: all rows of n images filtered
// in one launch (filtered[i]: height[i] * (rowBytes[i] + 1) bytes on the device) ...
inline void PngFilterBatchDevice(const std::vector<const void *> &pixels, const std::vector<int64_t> &rowBytes, const std::vector<int64_t> &height,
                                 const std::vector<int> &bytesPerPixel, const std::vector<int> &filter, const std::vector<void *> &filtered,
                                 zs_ctx *ctx = nullptr, void *hipStream = nullptr) {
    const size_t n = pixels.size();
    if (rowBytes.size() != n || height.size() != n || bytesPerPixel.size() != n || filter.size() != n || filtered.size() != n)
        throw ZlibStreamException("png: the argument lists differ in length");
    zs_ctx *c = ctx ? ctx : GpuContext::Shared();
    if (zs_png_filter_batch_device(c, (int)n, pixels.data(), rowBytes.data(), height.data(), bytesPerPixel.data(), filter.data(), filtered.data(),
                                   hipStream) != ZS_OK)
        throw ZlibStreamException("png: bad arguments");
}
// ... and n device-resident streams deflated in one call, stream i written in the NoFlush Writes whose cumulative ends are
// writeEnds[i] (empty: one Write).  Returns the streams' lengths.
inline std::vector<int64_t> DeflateWritesBatchDevice(const std::vector<const void *> &in, const std::vector<int64_t> &inLen,
                                                     const std::vector<std::vector<int64_t>> &writeEnds, const std::vector<void *> &out,
                                                     const std::vector<int64_t> &outCap, CompressionLevel level = CompressionLevel::DefaultCompression,
                                                     CompressionStrategy strategy = CompressionStrategy::DefaultStrategy, zs_ctx *ctx = nullptr,
                                                     void *hipStream = nullptr) {
    const size_t n = in.size();
    if (inLen.size() != n || writeEnds.size() != n || out.size() != n || outCap.size() != n)
        throw ZlibStreamException("deflating: the argument lists differ in length");
    zs_ctx *c = ctx ? ctx : GpuContext::Shared();
    std::vector<const int64_t *> lists(n, nullptr);
    std::vector<int64_t> counts(n, 0), outLen(n, 0);
    for (size_t i = 0; i < n; i++)
        if (!writeEnds[i].empty()) lists[i] = writeEnds[i].data(), counts[i] = (int64_t)writeEnds[i].size();
    const int rc = zs_deflate_writes_batch_device(c, (int)n, in.data(), inLen.data(), lists.data(), counts.data(), out.data(), outCap.data(), outLen.data(),
                                                  nullptr, (int)level, (int)strategy, 0, hipStream);
    if (rc != ZS_OK) throw ZlibStreamException(std::string("deflating: ") + zs_ctx_last_error(c));
    return outLen;
}

// ZlibOutputStream.cs: write-only stream that deflates into BaseStream.
class ZlibOutputStream {
public:
    static constexpr int BufferSize = 512;  // ZlibOutputStream.cs: chunkBuffer

    ZlibOutputStream(std::ostream &output, CompressionLevel level, zs_ctx *ctx = nullptr)
        : ZlibOutputStream(output, ZlibOptions{level, CompressionStrategy::DefaultStrategy, FlushMode::NoFlush}, ctx) {}

    ZlibOutputStream(std::ostream &output, const ZlibOptions &options, zs_ctx *ctx = nullptr) : BaseStream(output), Options(options) {
        // ZlibStream.cs:18-29: a null level means inflate mode -- the stream inflates what is written to it
        compress_ = Options.CompressionLevel_.has_value();
        if (compress_) {
            // Deflate..ctor throws ArgumentOutOfRangeException (Deflate.cs:258-281)
            z_ = zs_deflate_init(ctx ? ctx : GpuContext::Shared(), (int)*Options.CompressionLevel_, (int)Options.CompressionStrategy_, 15, 8,
                                 ZS_HASH_CRC32C);
            if (!z_) throw std::out_of_range("level / strategy");
        } else {
            zi_ = zs_inflate_init(ctx ? ctx : GpuContext::Shared(), 15);
            if (!zi_) throw std::out_of_range("windowBits");
        }
    }
    ZlibOutputStream(const ZlibOutputStream &) = delete;
    ZlibOutputStream &operator=(const ZlibOutputStream &) = delete;
    ~ZlibOutputStream() {
        try {
            Dispose();
        } catch (...) {
        }
    }

    std::ostream &BaseStream;
    ZlibOptions Options;
    long long TotalIn() const { return totalIn_; }
    long long TotalOut() const { return totalOut_; }
    bool CanRead() const { return false; }
    bool CanSeek() const { return false; }
    bool CanWrite() const { return true; }

    void WriteByte(uint8_t value) { Write(&value, 0, 1); }

    // WriteCore (ZlibOutputStream.cs:125-168)
    void Write(const uint8_t *buffer, int offset, int count) {
        if (!buffer && count) throw std::invalid_argument("buffer");
        if (count == 0) return;
        Loop(buffer + offset, count, (int)Options.FlushMode_);
    }
    void Write(const std::vector<uint8_t> &buffer) { Write(buffer.data(), 0, (int)buffer.size()); }

    void Flush() { BaseStream.flush(); }

    // Finish (ZlibOutputStream.cs:213-256) + Dispose (:186-211)
    void Dispose() {
        if (isDisposed_) return;
        isDisposed_ = true;
        try {
            if (!isFinished_) {
                Loop(nullptr, 0, ZS_FINISH);
                isFinished_ = true;
                Flush();
            }
        } catch (...) {
            End();
            throw;
        }
        End();
    }

private:
    void Loop(const uint8_t *in, int count, int flush) {
        int32_t availIn = count;
        const uint8_t *next = in;
        for (;;) {
            int32_t availOut = BufferSize;
            int32_t before = availIn;
            int state = compress_ ? zs_deflate(z_, next, &availIn, chunk_, &availOut, flush, &adler_, &totalIn_, &totalOut_)
                                  : zs_inflate(zi_, next, &availIn, chunk_, &availOut, flush, &adler_, &totalIn_, &totalOut_);
            next += before - availIn;
            if (state != ZS_OK && state != ZS_STREAM_END) {
                const char *m = compress_ ? zs_last_message(z_) : zs_inflate_message(zi_);
                throw ZlibStreamException(std::string(compress_ ? "deflating: " : "inflating: ") + (m ? m : ""));  // ThrowHelper.cs:21-23
            }
            if (BufferSize - availOut > 0) BaseStream.write((const char *)chunk_, BufferSize - availOut);
            if (!compress_ && availIn == 0 && availOut == 0 && flush != ZS_FINISH) break;  // ZlibOutputStream.cs:155-158
            if (state == ZS_STREAM_END) break;
            if (!(availIn > 0 || availOut == 0)) break;
        }
    }
    void End() {
        if (z_) zs_deflate_end(z_);
        if (zi_) zs_inflate_end(zi_);
        z_ = nullptr, zi_ = nullptr;
    }
    zs_deflate_stream *z_ = nullptr;
    zs_inflate_stream *zi_ = nullptr;
    bool compress_ = true;
    uint8_t chunk_[BufferSize];
    uint32_t adler_ = 1;
    int64_t totalIn_ = 0, totalOut_ = 0;
    bool isFinished_ = false, isDisposed_ = false;
};

// ZlibInputStream.cs: read-only stream that inflates BaseStream.  The device decodes whole streams: the
// first Read drains the base stream, inflates it on the GPU and later Reads are served from the result.
class ZlibInputStream {
public:
    // ZlibInputStream.cs:29-76: 8 KiB chunk buffer, inflate mode
    explicit ZlibInputStream(std::istream &input, zs_ctx *ctx = nullptr)
        : BaseStream(input), ctx_(ctx ? ctx : GpuContext::Shared()), z_(zs_inflate_init(ctx_, 15)), chunk_(8192) {
        if (!z_) throw std::out_of_range("windowBits");
    }
    ~ZlibInputStream() { zs_inflate_end(z_); }
    ZlibInputStream(const ZlibInputStream &) = delete;
    ZlibInputStream &operator=(const ZlibInputStream &) = delete;
    std::istream &BaseStream;
    bool CanRead() const { return true; }
    bool CanWrite() const { return false; }
    int64_t TotalIn() const { return totalIn_; }
    int64_t TotalOut() const { return totalOut_; }

    // ReadCore (ZlibInputStream.cs:133-186): refill the chunk buffer when it is empty, call Inflate while the caller's
    // buffer has room and the state is ZOK.  Returns the number of bytes read, 0 at the end of the stream.
    int Read(uint8_t *buffer, int offset, int count) {
        if (count == 0) return 0;
        int32_t availOut = count;
        uint8_t *nextOut = buffer + offset;
        int state;
        do {
            if (availIn_ == 0 && !noMoreInput_) {
                BaseStream.read(reinterpret_cast<char *>(chunk_.data()), (std::streamsize)chunk_.size());
                availIn_ = (int32_t)BaseStream.gcount();
                nextIn_ = 0;
            }
            const int32_t inBefore = availIn_, outBefore = availOut;
            state = zs_inflate(z_, chunk_.data() + nextIn_, &availIn_, nextOut, &availOut, ZS_NO_FLUSH, &adler_, &totalIn_, &totalOut_);
            nextIn_ += inBefore - availIn_;
            nextOut += outBefore - availOut;
            if (state != ZS_OK && state != ZS_STREAM_END) {
                const char *m = zs_inflate_message(z_);
                throw ZlibStreamException(std::string("inflating: ") + (m ? m : ""));  // ThrowHelper.cs:21-23
            }
        } while (availOut > 0 && state == ZS_OK);
        return count - availOut;
    }
    int ReadByte() {
        uint8_t b;
        return Read(&b, 0, 1) == 1 ? b : -1;
    }

private:
    zs_ctx *ctx_;
    zs_inflate_stream *z_;
    std::vector<uint8_t> chunk_;
    int32_t availIn_ = 0, nextIn_ = 0;
    bool noMoreInput_ = false;
    uint32_t adler_ = 1;
    int64_t totalIn_ = 0, totalOut_ = 0;
};

}  // namespace ZlibStream
}  // namespace SixLabors
