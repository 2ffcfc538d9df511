/*
 * zsgpu.h -- C ABI of the MI355X (gfx950) deflate engine for SixLabors/ZlibStream.
 *
 * The reference has no native boundary today (it is 100 % managed C#).  The
 * seam this library replaces is the zlib-style pair inside the reference's
 * internal z_stream facade:
 *
 *     CompressionState ZLibStream.Deflate(FlushMode)   src/ZlibStream/ZlibStream.cs:164-167
 *       -> Deflate.Compress(ZLibStream, FlushMode)     src/ZlibStream/Deflate.cs:436-636
 *     CompressionState ZLibStream.Inflate(FlushMode)   src/ZlibStream/ZlibStream.cs:119-122
 *       -> Inflate.Decompress(ZLibStream, FlushMode)   src/ZlibStream/Inflate.cs:103-357
 *
 * i.e. ZlibOutputStream / ZlibInputStream keep their public surface and their
 * WriteCore / Finish / ReadCore loops (ZlibOutputStream.cs:125-168, 213-256,
 * ZlibInputStream.cs:133-186); the engine object behind them is this library.
 * INTEGRATION.md shows the P/Invoke stub.
 *
 * Conventions: plain C, no C++ or torch types; return values are the
 * reference's CompressionState codes (CompressionState.cs); all pointers are
 * used only for the duration of the call unless stated otherwise (the
 * reference pins caller spans only inside WriteCore/ReadCore).
 *
 * There is NO CPU fallback: every entry point that compresses fails with
 * ZS_STREAM_ERROR and a message when no gfx950 device is usable.
 */
#ifndef ZSGPU_H
#define ZSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define ZS_API __declspec(dllexport)
#else
#define ZS_API __attribute__((visibility("default")))
#endif

/* CompressionState.cs */
enum {
    ZS_VERSION_ERROR = -6,
    ZS_BUF_ERROR = -5,
    ZS_MEM_ERROR = -4,
    ZS_DATA_ERROR = -3,
    ZS_STREAM_ERROR = -2,
    ZS_ERRNO = -1,
    ZS_OK = 0,
    ZS_STREAM_END = 1,
    ZS_NEED_DICT = 2
};
/* FlushMode.cs */
enum { ZS_NO_FLUSH = 0, ZS_PARTIAL_FLUSH = 1, ZS_SYNC_FLUSH = 2, ZS_FULL_FLUSH = 3, ZS_FINISH = 4 };
/* CompressionStrategy.cs */
enum { ZS_DEFAULT_STRATEGY = 0, ZS_FILTERED = 1, ZS_HUFFMAN_ONLY = 2, ZS_RLE = 3, ZS_FIXED = 4 };
/* Deflate.Intrinsics.cs:295-307: which UpdateHash the managed build would take */
enum { ZS_HASH_CRC32C = 0, ZS_HASH_MUL = 1 };

/* ------------------------------------------------------------------ */
/* Engine context: one per GPU (device ordinal as seen by HIP).  Owns the HIP
 * stream-ordered workspace that is reused across calls.  Not thread-safe;
 * distinct contexts are independent (as distinct reference Deflate instances
 * are, Deflate.Buffers.cs). */
typedef struct zs_ctx zs_ctx;

ZS_API int zs_ctx_create(int device, zs_ctx **out);
ZS_API void zs_ctx_destroy(zs_ctx *ctx);
ZS_API const char *zs_ctx_last_error(const zs_ctx *ctx);

/* Upper bound of the zlib stream produced for n input bytes. */
ZS_API int64_t zs_deflate_bound(int64_t n);

/* ------------------------------------------------------------------ */
/* Throughput entry points: n independent buffers, each compressed exactly as
 *     using (var s = new ZlibOutputStream(dst, level)) s.Write(buf, 0, len);
 * does (one Write of the whole buffer, then Dispose -> Finish;
 * ZlibOutputStream.cs:114-168,186-256; DeflateCorpusBenchmark.cs:86-100).
 *
 * _device: in[i] / out[i] are DEVICE pointers on ctx's GPU (inputs already
 * resident in HBM); `hip_stream` is a hipStream_t (NULL = the context's own
 * stream).  out_len[i] is a HOST array; the call returns after the results
 * are known (it synchronises the stream once).
 * Returns ZS_OK, or the first failing stream's code; per-stream codes are in
 * status[i] when status != NULL (ZS_BUF_ERROR when out_cap[i] is too small). */
ZS_API int zs_deflate_batch_device(zs_ctx *ctx, int n, const void *const *in, const int64_t *in_len, void *const *out,
                                   const int64_t *out_cap, int64_t *out_len, int *status, int level, int strategy,
                                   int hash_variant, void *hip_stream);

/* One stream written in several NoFlush Writes, resident in HBM:
 *     using (var s = new ZlibOutputStream(dst, level)) foreach (var w in writes) s.Write(w);
 * (ZlibOutputStream.cs:114-168: every Write is a call of Deflate(NoFlush), and every Write end a read event of
 * Fill_window, Deflate.cs:967-1019, which changes the bytes).  write_ends: the n_writes cumulative Write ends (HOST
 * array, increasing, the last one = in_len).  What zs_deflate does at Finish for the Writes it has buffered, without
 * the per-call protocol: the entry an encoder that has its image on the device (zs_png_filter_device) writes rows with. */
ZS_API int zs_deflate_writes_device(zs_ctx *ctx, const void *in, int64_t in_len, const int64_t *write_ends, int64_t n_writes,
                                    void *out, int64_t out_cap, int64_t *out_len, int level, int strategy, int hash_variant,
                                    void *hip_stream);

/* n independent streams, each written in its own NoFlush Writes: zs_deflate_writes_device for a batch, one call.
 * write_ends / n_writes are HOST arrays of n entries; write_ends[i] holds stream i's n_writes[i] cumulative Write ends
 * (non-decreasing, the last one = in_len[i]; an empty Write is dropped, as ZlibOutputStream drops it).
 * write_ends[i] == NULL, n_writes[i] <= 0 or a list that leaves one distinct end: the stream is one Write (a list of one
 * end is still checked against in_len[i]; zs_deflate_writes_device, which has no "no list", rejects n_writes == 0 for a
 * non-empty input).
 * write_ends == NULL: the call is zs_deflate_batch_device.  A malformed list anywhere is ZS_STREAM_ERROR for the whole
 * call, before any device work.  out_len / status / sub-batches / the one synchronisation at the end: as
 * zs_deflate_batch_device (ZS_BUF_ERROR for a stream whose out_cap is too small, the others unaffected).
 * One exception that leaves the bytes alone: at levels 1-3 a list-less stream of 256 KiB .. 4 MiB in a batch of at most 16
 * is not probed for the speculative runs (periodic data) once any stream of the call has a list; it takes the sweeps.
 * Every stream takes the path it takes alone through zs_deflate_writes_device -- also the slow one: a stream written
 * a few bytes at a time, and at levels 1-3 a stream with a Write end within 261 bytes below a window end (scanline
 * Writes often have one), runs on the one-wave literal engine whatever its neighbours are. */
ZS_API int zs_deflate_writes_batch_device(zs_ctx *ctx, int n, const void *const *in, const int64_t *in_len,
                                          const int64_t *const *write_ends, const int64_t *n_writes, void *const *out,
                                          const int64_t *out_cap, int64_t *out_len, int *status, int level, int strategy,
                                          int hash_variant, void *hip_stream);

/* Host-pointer form: copies in over PCIe, runs the device path, copies out. */
ZS_API int zs_deflate_batch(zs_ctx *ctx, int n, const void *const *in, const int64_t *in_len, void *const *out,
                            const int64_t *out_cap, int64_t *out_len, int *status, int level, int strategy,
                            int hash_variant);

/* Inflate (Inflate.Decompress, Inflate.cs:103-357; InflateBlocks.cs; InfCodes.cs; InfTree.cs): n independent
 * zlib streams, each decoded completely (what `new ZlibInputStream(src).Read(...)` to the end of the stream
 * yields, ZlibInputStream.cs:133-186).  out_cap[i] must hold the whole output.  status[i] is ZS_STREAM_END on
 * success; ZS_DATA_ERROR / ZS_BUF_ERROR / ZS_NEED_DICT with the reference's message in zs_ctx_last_error
 * otherwise (e.g. "incorrect data check", Inflate.cs:339).  Returns ZS_OK when every stream ended cleanly, else the
 * code of the first failing stream in the caller's order; zs_ctx_last_error is that same stream's message, whichever
 * of the library's paths decoded it.  A failing stream fails for itself only: its neighbours are complete.
 * out_len[i] of a failing stream: the bytes of the tokens (a literal, a whole match, a whole stored block) that were
 * decoded in full before the failure and fitted out_cap[i]; out[i][0 .. out_len[i]) holds them, and they are a prefix
 * of what the stream would have given.  So 0 for a refused header, the whole output for a bad Adler-32, and for a
 * truncated stream or a short out_cap[i] (ZS_BUF_ERROR, "buffer error") everything in front of the token that the
 * input or the room ended in -- never more than out_cap[i].  Bytes of out[i] behind out_len[i], up to out_cap[i], are
 * unspecified; nothing is written at or behind out[i] + out_cap[i]. */
ZS_API int zs_inflate_batch_device(zs_ctx *ctx, int n, const void *const *in, const int64_t *in_len, void *const *out,
                                   const int64_t *out_cap, int64_t *out_len, int *status, void *hip_stream);
ZS_API int zs_inflate_batch(zs_ctx *ctx, int n, const void *const *in, const int64_t *in_len, void *const *out,
                            const int64_t *out_cap, int64_t *out_len, int *status);

/* ------------------------------------------------------------------ */
/* The three containers of a deflate body: zlib (RFC 1950: 2 header bytes, Adler-32), none (RFC 1951: a ZIP entry, an HTTP
 * "deflate" body as most servers send it), gzip (RFC 1952: a .gz file, a BGZF block, an HTTP "gzip" body). */
enum { ZS_WRAP_ZLIB = 0, ZS_WRAP_RAW = 1, ZS_WRAP_GZIP = 2 };

/* zs_inflate_batch_device for streams in container `wrap`; that call is this one with ZS_WRAP_ZLIB and in_used == NULL.
 * ZS_WRAP_RAW: the first block begins at bit 0 of in[i] and the stream ends with its final block's last bit; there is no
 *   trailer and no checksum, so a stream that ends with output that fits is ZS_STREAM_END whatever follows it.
 * ZS_WRAP_GZIP: in[i] holds one gzip member (and whatever follows it).  A header kernel reads the members' headers -- FEXTRA,
 *   FNAME, FCOMMENT and FHCRC, which is verified --, the inflate kernels decode from the body's offset (in[i] itself is what
 *   they load from, so an aligned buffer keeps its 16-byte loads), one CRC-32 launch runs over the outputs that decoded and
 *   gathers the trailers, and the host compares CRC-32 and ISIZE (the output's length mod 2^32).  The call waits for the
 *   stream once more than the zlib call for the headers, and once for the CRCs.
 * in_used (HOST array, may be NULL): the bytes of in[i] the stream occupies -- header, body up to a whole byte, trailer --,
 *   which is where the next ZIP entry or gzip member begins; 0 for a failing stream.
 * status / out_len / the guard behind out_cap / "a stream fails for itself only": as for zs_inflate_batch_device.  A gzip
 * member adds zlib's messages for its own errors: "incorrect header check" (the magic), "unknown compression method",
 * "unknown header flags set", "header crc mismatch", "incorrect data check" (the CRC-32), "incorrect length check" (ISIZE)
 * -- all ZS_DATA_ERROR, out_len 0 for a header's, the whole output for a trailer's -- and ZS_BUF_ERROR "buffer error" for a
 * member cut short anywhere, header and trailer included.  ZS_STREAM_ERROR: a wrap outside the three, and what
 * zs_inflate_batch_device rejects. */
ZS_API int zs_inflate_wrap_batch_device(zs_ctx *ctx, int n, const void *const *in, const int64_t *in_len, void *const *out,
                                        const int64_t *out_cap, int64_t *out_len, int64_t *in_used, int *status, int wrap,
                                        void *hip_stream);

/* Upper bound of what zs_deflate_wrap_batch_device writes for n input bytes: zs_deflate_bound(n) + 0, - 6 or + 12.
 * -1 for a negative n or a wrap outside the three.  Pure host code. */
ZS_API int64_t zs_wrap_bound(int64_t n, int wrap);

/* zs_deflate_batch_device into container `wrap`; with ZS_WRAP_ZLIB it is that call.  For the two others the zlib streams
 * are written into a buffer the context owns (zs_deflate_bound(in_len[i]) each, kept until zs_ctx_destroy) and one framing
 * launch (KC's span copy) moves bytes [2, L - 4) of every stream that fits to out[i]: the compressed
 * bytes are read and written once more than by the zlib call.  The body is, bit for bit, the reference's NoHeader stream
 * (Deflate.cs:235-289, 622-634).  ZS_WRAP_GZIP puts 1f 8b 08 00, MTIME 0, XFL (2 at level 9, 4 at level 1, else 0) and OS
 * 255 in front, and behind the body the CRC-32 of in[i] -- computed by the same launch -- and in_len[i] mod 2^32.
 * out_len[i]: the bytes written, or, with status[i] == ZS_BUF_ERROR, the bytes out_cap[i] would have had to hold: nothing
 * is written for such a stream, the others are complete, and nothing is ever written at or behind out[i] + out_cap[i].
 * Everything else -- arguments, return value, ZS_STREAM_ERROR -- as for zs_deflate_batch_device; the call waits for the
 * stream once more than that call. */
ZS_API int zs_deflate_wrap_batch_device(zs_ctx *ctx, int n, const void *const *in, const int64_t *in_len, void *const *out,
                                        const int64_t *out_cap, int64_t *out_len, int *status, int level, int strategy,
                                        int hash_variant, int wrap, void *hip_stream);

/* What the first member of a gzip file says, and for a BGZF file (SAM/BAM specification 4.1: every member carries the
 * subfield SI1 = 66, SI2 = 67, SLEN = 2 with its own size minus one) what the walk over the members' sizes finds. */
typedef struct zs_gzip_info {
    int bgzf;            /* the first member carries the BGZF subfield */
    int xfl, os;         /* the first member's */
    uint32_t mtime;
    int64_t n_members;   /* BGZF: members, the empty end-of-file member included; otherwise -1 (only decoding tells) */
    int64_t name_off, name_len; /* the first member's FNAME without its terminator; 0 / 0: none */
    int64_t isize_sum;   /* BGZF: the sum of the members' ISIZE words = the decoded length; otherwise -1 */
} zs_gzip_info;

/* One file in HOST memory, pure host code, no context and no GPU.  ZS_OK and *info; ZS_DATA_ERROR for a first header that is
 * not gzip's (magic, method, reserved flags, FHCRC) and for a BGZF file whose walk meets a header it cannot read or a member
 * without the subfield; ZS_BUF_ERROR for a first header cut short and for a BGZF member whose size points past the end of
 * the file; ZS_STREAM_ERROR for null pointers or a negative len.  Zero bytes behind the last member are stepped over. */
ZS_API int zs_gzip_file_info(const void *file, int64_t len, zs_gzip_info *info);

/* gzip files to bytes, n files a call: what gzip(1) gives, the members of a file decoded back to back into out[i] (DEVICE
 * pointer, out_cap[i] bytes).  file[i] / file_len[i]: whole files in HOST memory; they go to the device in one copy.
 * A BGZF file is walked on the host by its members' sizes: every member of every such file of the call is one stream of one
 * zs_inflate_wrap_batch_device launch, its place in out[i] the sum of the ISIZE words in front of it; a member whose decoded
 * length is not its ISIZE fails its file with "incorrect length check".  The other files go in rounds: round r decodes
 * member r of every file that still has bytes, from where the member before ended, one inflate call a round.  Zero bytes
 * behind the last member are accepted; anything else there is "incorrect header check".
 * out_len[i]: the bytes decoded, for a failing file those of the members in front of the one that failed (BGZF: in front of
 * the first that failed).  n_members (HOST, may be NULL): members decoded.  status[i] (may be NULL): ZS_OK, or the failing
 * member's code; a file fails for itself only, and zs_ctx_last_error names the first failing file and the reason.
 * Returns ZS_OK, the first failing file's code, ZS_MEM_ERROR, or, before any device work, ZS_STREAM_ERROR: null context,
 * n < 0, null arrays or pointers, a negative length or capacity, a file or capacity above 2 GiB - 1 KiB. */
ZS_API int zs_gzip_decode_files_batch(zs_ctx *ctx, int n, const void *const *file, const int64_t *file_len, void *const *out,
                                      const int64_t *out_cap, int64_t *out_len, int *n_members, int *status, void *hip_stream);

/* ------------------------------------------------------------------ */
/* ZIP archives (PKWARE APPNOTE 6.3; .zip, .docx, .jar, .npz, .whl): whole files decoded on the device, and archives written
 * there.  The container's rules are zlibstream_amd/csrc/zs_zip.h's:
 *   - the end record is searched backwards over the last 22 + 65535 bytes; the first signature whose comment length reaches
 *     exactly the end of the file is taken.  No such record: ZS_DATA_ERROR (ZS_BUF_ERROR for a file under 22 bytes);
 *   - the ZIP64 end record and the ZIP64 extra field (id 0x0001: size, compressed size, local offset) are read where a field
 *     is all ones;
 *   - shift = (place of the end record, or of the ZIP64 one) - cd_len - cd_off: bytes in front of the archive (a
 *     self-extractor) are added to every offset, as Python's zipfile does; a negative shift is ZS_DATA_ERROR;
 *   - ZS_DATA_ERROR for the file: "multi-disk archives are not supported" (a disk number other than 0, counts that differ),
 *     a central record without its signature or reaching out of the directory, records that do not end exactly at
 *     cd_off + cd_len, a record count that does not match;
 *   - per entry, the walk going on: flag bit 0, 6 or 13 -- ZS_DATA_ERROR "encrypted entries are not supported"; a method
 *     outside {0, 8} -- ZS_DATA_ERROR "unsupported compression method"; method 0 with comp_len != len -- ZS_DATA_ERROR
 *     "incorrect length check"; a local header without its signature or with another name than the central record's --
 *     ZS_DATA_ERROR "local header mismatch"; a local header or a body that the file ends in -- ZS_BUF_ERROR "buffer error".
 *     Flag bit 3 (a data descriptor behind the body) is legal and the descriptor is never read: sizes and CRC-32 are the
 *     central directory's.  The body begins behind the LOCAL header's name and extra field, which may differ from the
 *     central record's. */
enum { ZS_ZIP_AUTO = -1, ZS_ZIP_STORED = 0, ZS_ZIP_DEFLATED = 8 };

typedef struct zs_zip_info {
    int64_t n_entries, total_len;      /* total_len: the sum of the entries' len = what the decode call writes */
    int64_t cd_off, cd_len, shift;     /* as found, shift applied to cd_off */
    int64_t comment_off, comment_len;
    int zip64;                         /* a ZIP64 end record was used */
} zs_zip_info;

typedef struct zs_zip_entry {
    int64_t name_off; int name_len;    /* the central directory's copy of the name, in the file */
    int method, flags;
    uint32_t crc32;
    int64_t comp_len, len, local_off, body_off, out_off; /* local_off: shift applied; out_off: sum of len of the entries in front */
    uint16_t dos_time, dos_date; uint32_t external_attr;
    int status;                        /* ZS_OK: decodable; else why not (rules above), body_off undefined */
} zs_zip_entry;

/* One archive in HOST memory, pure host code, no context and no GPU.  ZS_OK, *info and the entries; the file's error (rules
 * above), with *info as far as the end record gave it; ZS_STREAM_ERROR for null pointers or negative lengths.  entries may be
 * NULL (entries_cap 0) to ask for the counts only; entries_cap < n_entries: ZS_BUF_ERROR with info filled and the first
 * entries_cap entries written. */
ZS_API int zs_zip_file_info(const void *file, int64_t len, zs_zip_info *info, zs_zip_entry *entries, int64_t entries_cap);

/* ZIP archives to their entries' bytes, n archives a call.  file[i] / file_len[i]: whole files in HOST memory; they go to
 * the device in one copy and are walked on the host.  out[i] (DEVICE pointer, out_cap[i] bytes): entry e of file i lands at
 * out[i] + out_off[e] (zs_zip_file_info gives the offsets), out_len[i] is total_len.  All deflated entries of all files are
 * the streams of one raw inflate launch, each with exactly len bytes of room: a body that needs more, or ends with fewer, is
 * ZS_DATA_ERROR "incorrect length check"; one that ends in front of comp_len is accepted, as zipfile accepts it.  One CRC-32
 * launch then copies every stored entry into place and checks all entries: ZS_DATA_ERROR "incorrect data check".
 * out_cap[i] < total_len: ZS_BUF_ERROR for that file, nothing of it is decoded, out_len[i] says what it needs.  total_len or
 * the file above 2 GiB - 1 KiB: ZS_DATA_ERROR for that file (take the offsets from zs_zip_file_info and call the raw inflate).
 * entry_status (HOST, may be NULL, as may entry_status[i]): n_entries ints per file, ZS_OK or the entry's code; written only
 * for a file whose directory was walked and whose out_cap sufficed.  status[i] (may be NULL): ZS_OK, the file's error, or
 * its first failing entry's code; zs_ctx_last_error names the first failing file, the entry and the reason ("file 1: entry 2:
 * incorrect data check").  A failing entry's bytes are unspecified, every other entry is complete, and nothing is written
 * outside [out[i], out[i] + total_len).  Returns ZS_OK, the first failing file's code, ZS_MEM_ERROR, or, before any device
 * work, ZS_STREAM_ERROR: null context, n < 0, null arrays or pointers, a negative length or capacity.  The call waits for
 * the stream for the upload, as the inflate call does, and once for the CRCs. */
ZS_API int zs_zip_decode_files_batch(zs_ctx *ctx, int n, const void *const *file, const int64_t *file_len, void *const *out,
                                     const int64_t *out_cap, int64_t *out_len, int *const *entry_status, int *status,
                                     void *hip_stream);

typedef struct zs_zip_put {
    const void *data; int64_t len;     /* DEVICE pointer (may be NULL where len is 0), 0 .. 2 GiB - 1 KiB */
    const char *name; int name_len;    /* HOST bytes, 1 .. 65535, written as given */
    int method;                        /* ZS_ZIP_AUTO, ZS_ZIP_STORED, ZS_ZIP_DEFLATED */
    int utf8;                          /* general purpose bit 11 */
    uint16_t dos_time, dos_date;       /* written as given (0 / 0x0021 = 1980-01-01 00:00 is a sane default) */
    uint32_t external_attr;            /* "made by" host byte 3 (Unix) when its high 16 bits are non-zero, else 0 */
} zs_zip_put;

/* Room that zs_zip_encode_batch_device needs for these entries at the most: 22 + per entry 76 + 2 name_len + len, and for
 * an entry forced to ZS_ZIP_DEFLATED zs_wrap_bound(len, ZS_WRAP_RAW) in place of len.  Pure host code.  -1 for what that
 * call refuses: n_entries outside 0 .. 65535, a null list, a field of a zs_zip_put out of range, a bound above 2^32 - 1. */
ZS_API int64_t zs_zip_bound(const zs_zip_put *entries, int n_entries);

/* Entries in device memory to ZIP archives in device memory, n archives a call: archive i holds entries[i][0 .. n_entries[i]).
 * Its bytes: per entry a local header (version needed 20, or 10 for a stored entry, no extra field, no data descriptor),
 * the name and the body; the central directory; the end record without a comment.  ZIP64 is not written.
 * One zs_deflate_batch_device call deflates every entry of every archive that is not ZS_ZIP_STORED or empty, into a buffer the
 * context owns; a deflated body is, bit for bit, what zs_deflate_wrap_batch_device(..., ZS_WRAP_RAW) writes for the same bytes,
 * level, strategy and hash variant.  ZS_ZIP_AUTO keeps the stored form when the raw body is not shorter than the data; an
 * empty entry is always stored.  One framing launch (KC) then copies headers, names, bodies and directories into place and
 * computes the CRC-32 of every entry's data, and a closing kernel writes each into its local header and central record: the
 * CRCs never come to the host.  The call waits for the stream once more than the deflate call.
 * out_len / out_cap / status / the return value: as for zs_deflate_wrap_batch_device -- an archive that does not fit is
 * ZS_BUF_ERROR, out_len[i] says what it needs, nothing is written for it and the others are complete; zs_zip_bound is always
 * enough.  ZS_STREAM_ERROR before any device work for what zs_zip_bound answers with -1, and for null arrays or pointers. */
ZS_API int zs_zip_encode_batch_device(zs_ctx *ctx, int n, const zs_zip_put *const *entries, const int *n_entries,
                                      void *const *out, const int64_t *out_cap, int64_t *out_len, int *status, int level,
                                      int strategy, int hash_variant, void *hip_stream);

/* ------------------------------------------------------------------ */
/* TIFF files with Deflate compression (TIFF 6.0; compression 8, Adobe's, and 32946, the older code for the same): whole files
 * decoded on the device, and files written there.  A Deflate TIFF is a batch of independent zlib streams, one per strip or
 * tile ("chunk" below), with an optional predictor in front.  The container's rules are zlibstream_amd/csrc/zs_tiff.h's:
 *   - read: classic TIFF (42) and BigTIFF (43), "II" and "MM"; a page is an IFD of the chain (SubIFDs are not followed); tags
 *     256, 257, 258, 259, 262, 266, 273, 274, 277, 278, 279, 284, 317, 322, 323, 324, 325, 338, 339, their values as BYTE, SHORT,
 *     LONG or LONG8, with the specification's defaults (RowsPerStrip 2^32 - 1 = one strip);
 *   - accepted: compression 1 (none), 8, 32946; predictor 1, 2 (horizontal differencing; 8, 16 or 32 bits) and 3 (floating
 *     point; 32 bits, sample format 3); 1, 2, 4, 8, 16 or 32 bits per sample, the same for all; 1 .. 8 samples per pixel;
 *     planar configuration 1 (2 with one sample); strips, or tiles whose width and length are multiples of 16;
 *   - ZS_DATA_ERROR for the file, each with its own message: "not a TIFF file", "an IFD reaches out of the file", a tag's value
 *     that does, "the IFD chain loops", "no such page", "a required tag is missing" (256, 257, offsets, byte counts, and for
 *     tiles 322 and 323), offsets or byte counts that are not one per chunk, "unsupported compression method", "unsupported
 *     predictor", "unsupported planar configuration", "unsupported bits per sample", "unsupported samples per pixel",
 *     "unsupported fill order" (2), photometric 6 (YCbCr), "invalid strip or tile size", pixels above 2 GiB - 1 KiB;
 *   - ZS_BUF_ERROR: a file shorter than its header; per chunk, the walk going on, a body that the file ends in.
 * Photometric, ExtraSamples, SampleFormat and Orientation are reported, not interpreted. */
typedef struct zs_tiff_info {
    int64_t n_pages;                   /* IFDs in the chain */
    int big_endian, bigtiff;
    int64_t width, height;
    int bits, spp, sample_format, photometric;
    int extra_samples, extra_kind;     /* how many, and the first one's kind */
    int compression, predictor, planar, orientation;
    int tiled, pad;
    int64_t chunk_w, chunk_h, n_chunks; /* a tile; or the width and the rows of a strip */
    int64_t row_bytes, out_len;        /* ceil(width * spp * bits / 8), and height times that = what the decode call writes */
} zs_tiff_info;

typedef struct zs_tiff_chunk {
    int64_t off, comp_len;             /* the body in the file */
    int64_t x, y, w, h;                /* its place in the image, and the part of it that lies inside the image */
    int status, pad;                   /* ZS_OK, or ZS_BUF_ERROR: the file ends in it (off and comp_len are 0 then) */
} zs_tiff_chunk;

/* Page `page` of one file in HOST memory, pure host code, no context and no GPU.  ZS_OK, *info and the chunks; the file's
 * error (rules above), with n_pages and the byte order in *info as far as the walk got; ZS_STREAM_ERROR for null pointers or
 * negative numbers.  chunks may be NULL (chunks_cap 0) to ask for the counts only; chunks_cap < n_chunks: ZS_BUF_ERROR with
 * info filled and the first chunks_cap chunks written. */
ZS_API int zs_tiff_file_info(const void *file, int64_t len, int64_t page, zs_tiff_info *info, zs_tiff_chunk *chunks,
                             int64_t chunks_cap);

/* The predictor kernels alone (KT), n chunks a call, all pointers DEVICE pointers of any alignment.
 * Undo: in[i] is a decoded chunk, height[i] rows of ceil(width[i] * spp * bits / 8) bytes, as a TIFF reader has it behind
 * inflate; out[i] receives its top left out_width[i] x out_height[i] pixels (<= width, height: a tile that hangs over the
 * image's edge) as rows of ceil(out_width[i] * spp * bits / 8) bytes, samples little-endian.  Predictor 1 copies (and swaps
 * where big_endian[i], which may be NULL, says the samples lie most significant byte first), 2 sums every row with stride spp
 * mod 2^bits over the chunk's full width, 3 sums its bytes likewise and gathers the four byte planes, the most significant
 * first.  Predict is the inverse, and always little-endian: in[i] holds in_width[i] x in_height[i] pixels, out[i] receives
 * width[i] x height[i], the surplus filled by repeating the last pixel and the last row.
 * ZS_STREAM_ERROR before any device work: null arrays or pointers, a size outside 1 .. 2^31 - 1, a part larger than its
 * chunk, bits outside {1, 2, 4, 8, 16, 32}, spp outside 1 .. 8, predictor 2 below 8 bits, predictor 3 at other than 32, more
 * than 2^31 - 1 rows in the call.  n == 0 is ZS_OK.  With a hip_stream the launches stay in flight on it. */
ZS_API int zs_tiff_unpredict_batch_device(zs_ctx *ctx, int n, const void *const *in, void *const *out, const int64_t *width,
                                          const int64_t *height, const int64_t *out_width, const int64_t *out_height,
                                          const int *bits, const int *spp, const int *predictor, const int *big_endian,
                                          void *hip_stream);
ZS_API int zs_tiff_predict_batch_device(zs_ctx *ctx, int n, const void *const *in, void *const *out, const int64_t *in_width,
                                        const int64_t *in_height, const int64_t *width, const int64_t *height, const int *bits,
                                        const int *spp, const int *predictor, void *hip_stream);

/* TIFF files to pixels, n files a call.  file[i] / file_len[i]: whole files in HOST memory; they go to the device in one copy
 * and are walked on the host.  page (HOST, may be NULL: page 0 of every file): the page of file i.  out[i] (DEVICE pointer,
 * out_cap[i] bytes) receives height rows of row_bytes bytes, samples little-endian, out_len[i] is the page's out_len.
 * All deflated chunks of all files are the streams of one inflate launch, read from 16-byte-aligned pointers wherever they
 * lie in their files; their Adler-32s are checked by one more launch ("incorrect data check").  A strip must yield the rows
 * it has inside the image -- a last strip may also yield all of RowsPerStrip, both exist in the wild --, a tile all of itself:
 * fewer bytes, or more than the chunk holds, are ZS_DATA_ERROR "incorrect length check".  Strips of a file with predictor 1
 * whose samples need no swap are inflated straight into out[i]; every other chunk goes through a buffer the context owns and
 * one launch of the undo kernel, which also takes uncompressed chunks from the uploaded file.
 * out_cap[i] < out_len: ZS_BUF_ERROR for that file, nothing of it is decoded, out_len[i] says what it needs.  A file above
 * 2 GiB - 1 KiB: ZS_DATA_ERROR for that file.
 * chunk_status (HOST, may be NULL, as may chunk_status[i]): n_chunks ints per file, ZS_OK or the chunk's code; written only
 * for a file whose page was walked and whose out_cap sufficed.  status[i] (may be NULL): ZS_OK, the file's error, or its first
 * failing chunk's code; zs_ctx_last_error names the first failing file, the chunk and the reason ("file 1: chunk 7: incorrect
 * data check").  A failing chunk's pixels are unspecified, every other chunk is complete, and nothing is written outside
 * [out[i], out[i] + out_len).  Returns ZS_OK, the first failing file's code, ZS_MEM_ERROR, or, before any device work,
 * ZS_STREAM_ERROR: null context, n < 0, null arrays or pointers, a negative length, capacity or page. */
ZS_API int zs_tiff_decode_files_batch(zs_ctx *ctx, int n, const void *const *file, const int64_t *file_len, const int64_t *page,
                                      void *const *out, const int64_t *out_cap, int64_t *out_len, int *const *chunk_status,
                                      int *status, void *hip_stream);

typedef struct zs_tiff_put {
    const void *pixels;                /* DEVICE pointer: height rows of ceil(width * spp * bits / 8) bytes, little-endian */
    int64_t width, height;             /* 1 .. 2^31 - 1, the pixels at most 2 GiB - 1 KiB */
    int bits, spp;                     /* 1, 2, 4, 8, 16, 32; 1 .. 8 */
    int sample_format, photometric;    /* tags 339 and 262, written as given (photometric 6 is refused) */
    int extra_samples, extra_kind;     /* tag 338: how many of the spp samples are extra (0: the tag is left out), and their kind */
    int predictor, pad;                /* 1, 2 (bits >= 8), 3 (bits 32, sample format 3) */
    int64_t tile_width, tile_height;   /* multiples of 16; 0 / 0: strips */
    int64_t rows_per_strip;            /* 0: strips of about 256 KiB of pixels */
} zs_tiff_put;

/* Room that zs_tiff_encode_batch_device needs for this image at the most: the head (header, IFD, its longer values) and per
 * chunk zs_deflate_bound(its bytes) + 1.  Pure host code.  -1 for what that call refuses: a null pointer, a field out of range
 * (above), a bound above 2^32 - 1 (BigTIFF is not written). */
ZS_API int64_t zs_tiff_bound(const zs_tiff_put *put);

/* Images in device memory to TIFF files in device memory, n files a call: classic little-endian TIFF, one page, compression
 * 8, planar configuration 1, [header | IFD, tags ascending | the IFD's longer values | the chunks, each at an even offset].
 * One launch of the forward kernel cuts, pads and predicts every chunk of every image (a last strip is written with the rows
 * it has), one zs_deflate_batch_device call deflates them all into a buffer the context owns -- a chunk's stream is, bit for
 * bit, what that call writes for the same predicted bytes, level, strategy and hash variant --, the host builds the heads from
 * the lengths it returns, and one framing launch (KC's span copy) assembles the files.
 * out_len / out_cap / status / the return value: as for zs_zip_encode_batch_device -- a file that does not fit is
 * ZS_BUF_ERROR, out_len[i] says what it needs, nothing is written for it and the others are complete; zs_tiff_bound is always
 * enough.  ZS_STREAM_ERROR before any device work for what zs_tiff_bound answers with -1, and for null arrays or pointers. */
ZS_API int zs_tiff_encode_batch_device(zs_ctx *ctx, int n, const zs_tiff_put *puts, void *const *out, const int64_t *out_cap,
                                       int64_t *out_len, int *status, int level, int strategy, int hash_variant,
                                       void *hip_stream);

/* ------------------------------------------------------------------ */
/* OpenEXR files with ZIP / ZIPS compression: whole files decoded on the device into channel planes, and files written there.
 * Such a file is a batch of independent zlib streams, one per chunk of 1 (ZIPS) or 16 (ZIP) scanlines or per tile, with a
 * byte predictor over the whole chunk in front.  No third-party reader was at hand when this was written: the rules below,
 * which zlibstream_amd/csrc/zs_exr.h implements, are what the tests pin.
 *   File head.  Bytes 0-3 are 76 2F 31 01; bytes 4-7 a little-endian version word whose low byte must be 2.  Bit 0x200: single
 *     part, tiled.  Bit 0x400: long names, up to 255 bytes, otherwise 31.  Bit 0x800 (deep data), bit 0x1000 (multi-part) and
 *     every other bit are refused.  All integers and samples in the file are little-endian.
 *   Header.  Attributes: name\0 type\0 int32 size, then size bytes; a single \0 where a name would start ends the list.  Read:
 *     `channels` (chlist), `compression` (compression, 1 byte), `dataWindow` (box2i: xMin, yMin, xMax, yMax as int32,
 *     inclusive, negative values allowed), `lineOrder` (lineOrder, 1 byte: 0 increasing, 1 decreasing, 2 random, tiles only),
 *     with 0x200 `tiles` (tiledesc: uint32 xSize, uint32 ySize, a mode byte whose low nibble is 0 ONE_LEVEL, 1 MIPMAP,
 *     2 RIPMAP); `displayWindow` (box2i) is reported when present; every other attribute is stepped over.
 *   Channel list.  Per channel name\0, int32 type (0 UINT 4 bytes, 1 HALF 2 bytes, 2 FLOAT 4 bytes), uint8 pLinear, 3 reserved
 *     bytes, int32 xSampling, int32 ySampling; a \0 ends the list.  The file's layout order is the list's order (writers sort
 *     byte-wise, so RGBA lies as A, B, G, R; the reader does not demand it).
 *   Compression.  0 none, 2 ZIPS (1 line a chunk), 3 ZIP (16 lines a chunk); every other value (RLE 1, PIZ 4, PXR24 5, B44 6,
 *     B44A 7, DWAA 8, DWAB 9) is "unsupported compression method".
 *   Offset table.  Directly behind the header, one uint64 absolute file offset per chunk.  Scanlines: n = ceil(H / L), entry k
 *     is the chunk whose first line is yMin + k L whatever the line order (decreasing order only changes where the bodies
 *     lie).  ONE_LEVEL tiles: n = ceil(W / tx) ceil(H / ty), entry tileY * nx + tileX.
 *   Chunk.  Scanlines: int32 y, int32 dataSize, data.  Tiles: int32 tileX, tileY, levelX, levelY, int32 dataSize, data.  The
 *     coordinates must match the table slot.  The chunk's raw bytes U: for each row, for each channel in list order, w samples
 *     -- w the image's width or the part of the tile inside the data window; edge tiles and a last scanline chunk hold only
 *     the pixels and rows they have.  dataSize == U: the bytes lie raw (always so under compression 0; also what a writer
 *     does when zlib did not shrink the chunk).  dataSize < U: a zlib stream that must inflate to exactly U bytes t[0 .. U),
 *     which are undone in two steps: t[i] = (t[i-1] + t[i] - 128) mod 256 for i >= 1, then raw[2k] = t[k], raw[2k+1] = t[h+k]
 *     with h = (U + 1) / 2.  (Raw 01 02 03 04 05 is split 01 03 05 02 04 and stored 01 82 82 7D 82.)
 *   ZS_DATA_ERROR for the file, each with its own message: "not an OpenEXR file", an unsupported version, deep data,
 *     multi-part, other flag bits, "the header reaches out of the file", a name longer than the flags allow, an attribute
 *     whose size disagrees with its type (for the five read), "a required attribute is missing", an empty or inverted data
 *     window, no channels or more than 64, "unsupported pixel type", "unsupported channel sampling" (any sampling != 1),
 *     "unsupported level mode" (MIPMAP, RIPMAP), tile size 0, line order 2 on scanlines, "the offset table reaches out of the
 *     file", pixels above 2 GiB - 1 KiB.  Per chunk, the walk going on: "a chunk's coordinates do not match its place",
 *     "invalid chunk size" (dataSize > U or < 0).
 *   ZS_BUF_ERROR: a file shorter than 8 bytes; per chunk, the walk going on, an offset or body that the file ends in.
 * Output layout: channel-planar, the layout a tensor wants and the only one that holds mixed types.  Plane c is H rows of W
 * samples, little-endian, at plane_off[c]: the running sum of the planes' bytes, rounded up to 16; out_len is the end of the
 * last plane; the padding bytes between planes are never written.
 * Out of scope: tiles, decreasing order and long names on the write side; mip / rip levels; multi-part and deep files;
 * sampled channels; every codec but zlib; interleaved (H, W, C) output; the dotnet shim has no binding for these calls. */
typedef struct zs_exr_info {
    int32_t data_window[4], display_window[4];  /* xMin, yMin, xMax, yMax */
    int64_t width, height;
    int n_channels, compression, line_order, tiled;
    int has_display_window, long_names;
    int64_t tile_w, tile_h;             /* 0 for scanline files */
    int64_t lines_per_chunk, n_chunks;  /* 1 or 16, or a tile's height */
    int64_t out_len;                    /* what the decode call writes into */
} zs_exr_info;

typedef struct zs_exr_channel {
    char name[256];
    int type, sample_bytes;             /* 0 UINT, 1 HALF, 2 FLOAT; 4, 2, 4 */
    int64_t plane_off;
} zs_exr_channel;

typedef struct zs_exr_chunk {
    int64_t off, data_len, raw_len;     /* the data behind the chunk's header in the file (dataSize bytes), and U */
    int64_t x, y, w, h;                 /* its place, counted from the data window's corner */
    int status, pad;                    /* ZS_OK, ZS_BUF_ERROR or ZS_DATA_ERROR (rules above; off and data_len are 0 then) */
} zs_exr_chunk;

/* One file in HOST memory, pure host code, no context and no GPU.  ZS_OK, *info, the channels and the chunks; the file's error
 * (rules above) with *info as far as the walk got; ZS_STREAM_ERROR for null pointers or negative numbers.  channels and chunks
 * may be NULL (cap 0) to ask for the counts only; a cap below the count: ZS_BUF_ERROR with info filled and the first cap
 * entries written. */
ZS_API int zs_exr_file_info(const void *file, int64_t len, zs_exr_info *info, zs_exr_channel *channels, int64_t channels_cap,
                            zs_exr_chunk *chunks, int64_t chunks_cap);

/* The predictor kernels alone (KE), n chunks a call, DEVICE pointers of any alignment, len[i] in
 * 1 .. 2^31 - 1, contiguous in, contiguous out.  Undo: in[i] holds a chunk's inflated bytes t, out[i] receives its raw bytes
 * (both steps above).  Predict is the inverse.  ZS_STREAM_ERROR before any device work for null arrays or pointers or a length
 * out of range.  n == 0 is ZS_OK.  With a hip_stream the launches stay in flight on it. */
ZS_API int zs_exr_unpredict_batch_device(zs_ctx *ctx, int n, const void *const *in, void *const *out, const int64_t *len,
                                         void *hip_stream);
ZS_API int zs_exr_predict_batch_device(zs_ctx *ctx, int n, const void *const *in, void *const *out, const int64_t *len,
                                       void *hip_stream);

/* OpenEXR files to channel planes, n files a call.  file[i] / file_len[i]: whole files in HOST memory; they go to the device
 * in one copy and are walked on the host.  out[i] (DEVICE pointer, out_cap[i] bytes) receives the planes (layout above),
 * out_len[i] is the file's out_len.  All zlib chunks of all files are the streams of one inflate launch, read from
 * 16-byte-aligned pointers wherever they lie in their files, into a buffer the context owns; their Adler-32s are checked by
 * one more launch ("incorrect data check"); a stream that yields fewer or more than U bytes is ZS_DATA_ERROR "incorrect length
 * check".  One launch of the undo kernel over all chunks then writes the planes; chunks that lie raw come from the uploaded
 * file and take the same launch with both steps off.
 * out_cap[i] < out_len: ZS_BUF_ERROR for that file, nothing of it is decoded, out_len[i] says what it needs.  A file above
 * 2 GiB - 1 KiB: ZS_DATA_ERROR for that file.
 * chunk_status (HOST, may be NULL, as may chunk_status[i]): n_chunks ints per file, ZS_OK or the chunk's code; written only
 * for a file whose header was walked and whose out_cap sufficed.  status[i] (may be NULL): ZS_OK, the file's error, or its
 * first failing chunk's code; zs_ctx_last_error names the first failing file, the chunk and the reason ("file 1: chunk 7:
 * incorrect data check").  A failing chunk's pixels are unspecified, every other chunk is complete, and nothing is written
 * outside [out[i], out[i] + out_len).  Returns ZS_OK, the first failing file's code, ZS_MEM_ERROR, or, before any device work,
 * ZS_STREAM_ERROR: null context, n < 0, null arrays or pointers, a negative length or capacity. */
ZS_API int zs_exr_decode_files_batch(zs_ctx *ctx, int n, const void *const *file, const int64_t *file_len, void *const *out,
                                     const int64_t *out_cap, int64_t *out_len, int *const *chunk_status, int *status,
                                     void *hip_stream);

typedef struct zs_exr_put {
    const void *planes;                 /* DEVICE pointer: the channel planes, layout above */
    int64_t width, height;              /* 1 .. 2^31 - 1, the planes at most 2 GiB - 1 KiB */
    int32_t x_min, y_min;               /* the data window's corner; the display window is written equal to the data window */
    int n_channels, compression;        /* 1 .. 64; 0, 2 (ZIPS) or 3 (ZIP) */
    const char *const *names;           /* HOST: n_channels names of 1 .. 31 bytes, sorted byte-wise, none twice */
    const int *types;                   /* HOST: 0 UINT, 1 HALF, 2 FLOAT */
    const void *extra;                  /* HOST, may be NULL: attributes the caller has encoded, copied verbatim behind the others */
    int64_t extra_len;
} zs_exr_put;

/* Room that zs_exr_encode_batch_device needs for this image at the most: the head, the offset table, and per chunk its eight
 * bytes of header and its raw bytes (a chunk that zlib does not shrink is stored raw).  Pure host code.  -1 for what that
 * call refuses: a null pointer, a field out of range, names that are unsorted, repeated, empty or longer than 31 bytes. */
ZS_API int64_t zs_exr_bound(const zs_exr_put *put);

/* Channel planes in device memory to OpenEXR files in device memory, n files a call: single-part scanline files, version word
 * 02 00 00 00, increasing Y, the attributes channels, compression, dataWindow, displayWindow, lineOrder, pixelAspectRatio 1.0,
 * screenWindowCenter (0, 0), screenWindowWidth 1.0 and the extras, in this order.  One launch of the forward kernel gathers,
 * splits and differences every chunk, one zs_deflate_batch_device call deflates them all into a buffer the context owns -- a
 * deflated chunk is, bit for bit, what that call writes for the same predicted bytes, level, strategy and hash variant --,
 * the host reads the lengths, a chunk whose stream is not shorter than its raw bytes is stored raw (a second, small forward
 * launch with both steps off, for those chunks only), the host builds head, offset table and chunk headers, and one framing
 * launch (KC's span copy) assembles the files.
 * out_len / out_cap / status / the return value: as for zs_tiff_encode_batch_device -- a file that does not fit is
 * ZS_BUF_ERROR, out_len[i] says what it needs, nothing is written for it and the others are complete; zs_exr_bound is always
 * enough.  ZS_STREAM_ERROR before any device work for what zs_exr_bound answers with -1, and for null arrays or pointers. */
ZS_API int zs_exr_encode_batch_device(zs_ctx *ctx, int n, const zs_exr_put *puts, void *const *out, const int64_t *out_cap,
                                      int64_t *out_len, int *status, int level, int strategy, int hash_variant,
                                      void *hip_stream);

/* ------------------------------------------------------------------ */
/* Chunked N-dimensional arrays: the chunks of an HDF5 / NetCDF-4 dataset with the shuffle and deflate filters, and of a
 * Zarr v2 array with the `zlib` or `gzip` compressor and the `shuffle` filter, which are byte for byte the same thing.  No
 * file format is walked: the caller gives the geometry and the chunks (h5py read_direct_chunk / write_direct_chunk, a Zarr
 * store's values).  The rules, which tests/chunk_cases.py models and the tests pin:
 *   An array has rank 1..8, shape[d] >= 1, chunk[d] >= 1, elements of elem_size 1..16 bytes in C order (last axis fastest).
 *   grid[d] = ceil(shape[d] / chunk[d]); chunk c is the C-order index of its grid coordinates (Zarr's key i.j.k, HDF5's
 *   chunk offset divided by the chunk dims).
 *   A decoded chunk has E = prod(chunk[d]) elements, chunk_bytes = E * elem_size bytes, always: edge chunks are full-sized
 *   and padded.  Chunk element q (C order over chunk[]) of grid cell p is array element p[d] * chunk[d] + q[d]; it exists
 *   when that index is below shape[d] on every axis.  The others are padding: ignored when reading, written as `fill` (one
 *   element of elem_size bytes) when writing.
 *   Shuffle (H5Zshuffle, numcodecs Shuffle): byte j of element e lies at j * E + e of the chunk.  On a bare buffer of any
 *   length (the two stand-alone calls) count = len / elem_size, and the len % elem_size leftover bytes are copied unchanged
 *   behind the planes, which is HDF5's rule.
 *   wrap: ZS_WRAP_ZLIB is HDF5 deflate and numcodecs Zlib, ZS_WRAP_GZIP numcodecs GZip; ZS_WRAP_RAW is accepted too.
 *   Per-chunk flags: ZS_CHUNK_STORED -- the bytes are not compressed (HDF5's filter-mask bit of an optional deflate that did
 *   not shrink; a Zarr array with compressor null); ZS_CHUNK_UNSHUFFLED -- the filter-mask bit of the shuffle filter;
 *   ZS_CHUNK_SKIP (read side) -- this chunk was not fetched: its region is left alone; ZS_CHUNK_ABSENT (write side) -- the
 *   chunk was not written.  A chunk with a null pointer and no SKIP flag is missing: its region reads as `fill`.
 * Three more filters go through the _filters_ calls further down (zs_chunk_filters): Fletcher-32, delta and big-endian elements.
 * Out of scope: Fortran order; the filters scale-offset, bitshuffle, szip and N-bit; Blosc, LZ4 and Zstd; Zarr v3 and
 * sharding; Delta on floating-point dtypes and Delta whose astype differs from its dtype; numcodecs Fletcher32 as a Zarr
 * filter (its checksum sits inside the compressed stream); the byte-swapped checksum that HDF5 also accepts for files written
 * before 1.6.3; reading HDF5 files themselves; object and variable-length dtypes. */
enum { ZS_CHUNK_STORED = 1, ZS_CHUNK_UNSHUFFLED = 2, ZS_CHUNK_SKIP = 4, ZS_CHUNK_ABSENT = 8 };
enum { ZS_CHUNKS_SKIP_FILL = 1, ZS_CHUNKS_ALLOW_STORED = 2 };

typedef struct zs_chunk_grid {
    int rank;          /* 1..8 */
    int elem_size;     /* 1..16 */
    int64_t shape[8];  /* entries behind rank are not read */
    int64_t chunk[8];
    int shuffle;       /* 0 or 1: the chunks' bytes are shuffled (elem_size 1: the same bytes either way) */
    int wrap;          /* ZS_WRAP_* of the compressed chunks */
    uint8_t fill[16];  /* one element; bytes behind elem_size are not read */
} zs_chunk_grid;

typedef struct zs_chunk_ref {
    const void *data; /* HOST memory; NULL: the chunk is missing (or, with ZS_CHUNK_SKIP, was not fetched) */
    int64_t len;
    int flags;        /* ZS_CHUNK_STORED | ZS_CHUNK_UNSHUFFLED | ZS_CHUNK_SKIP */
} zs_chunk_ref;

/* n_chunks, chunk_bytes and array_bytes of a grid (each pointer may be NULL).  Pure host code.  ZS_STREAM_ERROR for a grid
 * that breaks a rule above -- rank, elem_size, an extent below 1, shuffle outside 0 / 1, wrap outside the three -- and for
 * products that leave int64. */
ZS_API int zs_chunk_grid_info(const zs_chunk_grid *grid, int64_t *n_chunks, int64_t *chunk_bytes, int64_t *array_bytes);

/* Chunks in host memory to arrays in device memory, n arrays a call.  chunks[i]: n_chunks(i) records in chunk order; out[i]:
 * DEVICE memory with array_bytes(i) of room.  One upload of all chunk bytes, one zs_inflate_wrap_batch_device call over all
 * compressed chunks of all arrays (one per container where the arrays of a call differ in `wrap`) into a buffer the context
 * owns -- exactly chunk_bytes of room per chunk, on 256-byte boundaries --, then one launch of the place kernel (KN,
 * DESIGN.md section 4) over the chunks that are whole: unshuffle and placement fused, STORED chunks read from the upload,
 * missing chunks written as `fill`.
 * A chunk fails for itself only: its code goes to chunk_status[i][c] (HOST arrays of n_chunks(i) ints; chunk_status or any
 * chunk_status[i] may be NULL), its region of out[i] is left untouched, its neighbours are complete.  Reasons: inflate's own
 * errors with their messages; ZS_BUF_ERROR "buffer error" for a stream that holds more than chunk_bytes; ZS_DATA_ERROR
 * "incorrect chunk length" for a stream that ends short of chunk_bytes and for a STORED chunk whose len != chunk_bytes.
 * status[i] (may be NULL): the first failing chunk's code, or ZS_OK; ZS_BUF_ERROR with nothing written for an array whose
 * out_cap[i] < array_bytes(i).  Nothing is ever written at or behind out[i] + out_cap[i].  Returns the first failing array's
 * code; zs_ctx_last_error names the array, the chunk and the reason ("array 1: chunk 7: incorrect data check").
 * ZS_STREAM_ERROR before any device work: null arguments, a bad grid, a negative length, a chunk_bytes or len above
 * 2 GiB - 1 KiB, more than 2^31 - 1 items (stretches of rows, zs_chunk.h) in the call.
 * The call waits for the stream for the upload, inside the inflate call, and for the place kernel's descriptors; with a
 * caller's hip_stream the place launch is left in flight on it. */
ZS_API int zs_chunks_decode_batch(zs_ctx *ctx, int n, const zs_chunk_grid *grids, const zs_chunk_ref *const *chunks, void *const *out,
                                  const int64_t *out_cap, int *const *chunk_status, int *status, void *hip_stream);

/* Room that zs_chunks_encode_batch_device needs for this array at the most: n_chunks * zs_wrap_bound(chunk_bytes, wrap).
 * Pure host code.  -1 for a bad grid and for a result that leaves int64. */
ZS_API int64_t zs_chunks_bound(const zs_chunk_grid *grid);

/* Arrays in device memory to their chunks in device memory, n arrays a call.  in[i]: the array; out[i] receives the chunks
 * back to back in chunk order: chunk c lies at out[i] + chunk_off[i][c] and has chunk_len[i][c] bytes, with
 * chunk_flags[i][c] (HOST arrays of n_chunks(i) entries; chunk_flags or any chunk_flags[i] may be NULL).  One launch of the
 * gather kernel (KN) reads every chunk's clipped region, pads it with `fill` and writes it, shuffled or not, into a buffer
 * the context owns; one deflate call over all chunks writes the streams into a second one -- a compressed chunk is, bit for
 * bit, what zs_deflate_wrap_batch_device writes for the same bytes, level, strategy, hash variant and wrap --; the host reads
 * the lengths, and one launch of KC's span copy moves the chunks into place (the pattern of zs_zip_encode_batch_device).
 * options & ZS_CHUNKS_SKIP_FILL: a survey launch (records per item, a folding launch, one more wait) finds the chunks whose
 *   existing elements all equal `fill`; such a chunk is not written: chunk_len 0, flag ZS_CHUNK_ABSENT, left out of gather
 *   and deflate.
 * options & ZS_CHUNKS_ALLOW_STORED: a chunk whose stream is not shorter than chunk_bytes is written as its (shuffled) bytes
 *   with flag ZS_CHUNK_STORED, HDF5's rule for an optional filter.  Without it every chunk is a stream, Zarr's rule.
 * An array whose out_cap[i] is short is left out: status[i] ZS_BUF_ERROR, out_len[i] what it needs, nothing written; the
 * others are complete, and zs_chunks_bound is always enough.  Returns the first failing array's code.  ZS_STREAM_ERROR
 * before any device work as for zs_chunks_decode_batch, and for unknown options. */
ZS_API int zs_chunks_encode_batch_device(zs_ctx *ctx, int n, const zs_chunk_grid *grids, const void *const *in, void *const *out,
                                         const int64_t *out_cap, int64_t *out_len, int64_t *const *chunk_off,
                                         int64_t *const *chunk_len, int *const *chunk_flags, int *status, int level, int strategy,
                                         int hash_variant, int options, void *hip_stream);

/* The shuffle filter alone on n device buffers (KN's gather and place kernels on a one-chunk, one-row array): out[i] =
 * the elem_size[i] planes of in[i]'s len[i] / elem_size[i] elements, the leftover bytes behind them; and the inverse.  in[i]
 * and out[i] must not overlap; any alignment; len[i] in 0 .. 2^31 - 1, elem_size[i] in 1..16. */
ZS_API int zs_shuffle_batch_device(zs_ctx *ctx, int n, const void *const *in, void *const *out, const int64_t *len,
                                   const int *elem_size, void *hip_stream);
ZS_API int zs_unshuffle_batch_device(zs_ctx *ctx, int n, const void *const *in, void *const *out, const int64_t *len,
                                     const int *elem_size, void *hip_stream);

/* Fletcher-32, the delta filter and big-endian elements: one zs_chunk_filters per array beside its zs_chunk_grid.  With every
 * field 0 the two _filters_ calls are the calls above: the same bytes, codes and messages.  The rules, which
 * tests/chunk_filter_cases.py models and the tests pin:
 *   byte_order 0 (little) or 1 (big).  The array on the device is always little-endian.  With 1 the chunks hold every
 *     element with its bytes reversed, and `fill`, given in the array's little-endian form, is written reversed into
 *     padding.  elem_size 1, 2, 4 or 8 (at 1 nothing changes); any other elem_size with byte_order 1 is ZS_STREAM_ERROR from
 *     the grid check.  With shuffle, plane j of a chunk is byte elem_size - 1 - j of the little-endian element.
 *   delta 0 or 1 (numcodecs Delta with astype equal to dtype, an integer dtype): elem_size 1, 2, 4 or 8, any other
 *     ZS_STREAM_ERROR.  Over the whole padded chunk of E elements in C order, wrapping on unsigned values of elem_size bytes:
 *     enc[0] = x[0], enc[k] = x[k] - x[k-1].  Encode order is delta, byte order, shuffle, deflate, and decode the inverse: with
 *     byte_order 1 the differences themselves are stored big-endian, as numcodecs does for Delta(dtype='>i4').  A STORED
 *     chunk still carries delta.
 *   fletcher32 0 or 1 (HDF5's last filter, fletcher32=True in h5py, NetCDF-4's checksum switch): computed over the chunk's
 *     bytes as they are stored -- the compressed stream, or the STORED bytes -- and appended as four little-endian bytes;
 *     len and chunk_len include them.  The checksum is H5_checksum_fletcher32: over the big-endian 16-bit words of the bytes
 *     (an odd last byte is a word with a zero low byte), s1 the sum of the words and s2 the sum of the running s1, each
 *     modulo 65535 with a residue of 0 reading as 0xffff unless every word is zero; (s2 << 16) | s1.
 *   reserved must be 0; a field outside its values is ZS_STREAM_ERROR.
 * Read side: a chunk with fletcher32 whose len < 4 is ZS_DATA_ERROR "incorrect chunk length", one whose checksum differs
 * ZS_DATA_ERROR "incorrect chunk checksum"; either fails for itself only and is not handed to inflate.  One launch of the
 * checksum kernel (KL) runs over all chunks where they lie behind the upload, and the host compares with the four bytes it
 * holds.  A chunk with delta goes from the inflate buffer (or the upload) through the delta kernels (KI: tile sums, a scan of
 * them, the tiles again), whose load side unshuffles and reverses, into a buffer of plain little-endian elements that the
 * place kernel takes; without delta the place kernel itself reverses.
 * Write side: gather with `fill`, delta (KI's encode kernel, which writes the byte order and the planes; without delta the
 * gather kernel does), deflate, the stored-or-stream choice and the span copy as above, then one KL launch over the placed
 * chunks whose fold writes the four bytes behind each. */
typedef struct zs_chunk_filters {
    int delta;      /* 0 or 1 */
    int byte_order; /* 0 little, 1 big */
    int fletcher32; /* 0 or 1 */
    int reserved;   /* must be 0 */
} zs_chunk_filters;

#define ZS_FLETCHER32_TILE 16384 /* bytes of a span that one wave sums (KL) */
#define ZS_DELTA_TILE 4096       /* elements of a buffer that one wave differences or sums (KI) */

/* zs_chunks_decode_batch with filters[i] for array i (n of them, not NULL). */
ZS_API int zs_chunks_decode_filters_batch(zs_ctx *ctx, int n, const zs_chunk_grid *grids, const zs_chunk_filters *filters,
                                          const zs_chunk_ref *const *chunks, void *const *out, const int64_t *out_cap,
                                          int *const *chunk_status, int *status, void *hip_stream);

/* zs_chunks_encode_batch_device with filters[i] for array i.  zs_chunks_filters_bound is always enough. */
ZS_API int zs_chunks_encode_filters_batch_device(zs_ctx *ctx, int n, const zs_chunk_grid *grids, const zs_chunk_filters *filters,
                                                 const void *const *in, void *const *out, const int64_t *out_cap, int64_t *out_len,
                                                 int64_t *const *chunk_off, int64_t *const *chunk_len, int *const *chunk_flags,
                                                 int *status, int level, int strategy, int hash_variant, int options,
                                                 void *hip_stream);

/* zs_chunks_bound(grid) + 4 * n_chunks with fletcher32.  Pure host code.  -1 for a bad grid, a bad pair of grid and filters
 * (rules above), a null pointer and a result that leaves int64. */
ZS_API int64_t zs_chunks_filters_bound(const zs_chunk_grid *grid, const zs_chunk_filters *filters);

/* Fletcher-32 (rules above) of n spans in DEVICE memory, any address, len[i] in 0 .. 2^31 - 1, into out (HOST, n words).  One
 * launch over the ZS_FLETCHER32_TILE-byte tiles of all spans and one that folds a span's tiles; the call waits for the
 * results. */
ZS_API int zs_fletcher32_batch_device(zs_ctx *ctx, int n, const void *const *in, const int64_t *len, uint32_t *out,
                                      void *hip_stream);

/* The delta filter alone on n device buffers of little-endian elements: count = len[i] / elem_size[i] elements, the
 * len % elem_size leftover bytes copied unchanged; elem_size[i] 1, 2, 4 or 8, len[i] in 0 .. 2^31 - 1, any alignment; in[i]
 * and out[i] must not overlap. */
ZS_API int zs_delta_encode_batch_device(zs_ctx *ctx, int n, const void *const *in, void *const *out, const int64_t *len,
                                        const int *elem_size, void *hip_stream);
ZS_API int zs_delta_decode_batch_device(zs_ctx *ctx, int n, const void *const *in, void *const *out, const int64_t *len,
                                        const int *elem_size, void *hip_stream);

/* ------------------------------------------------------------------ */
/* Multi-GPU batch entry points (SURVEY.md 8(b) "zs_deflate_batch(..., device_mask)", 8(e)): the n independent
 * buffers are partitioned over n_ctx contexts -- normally one per GPU of the node, zs_ctx_create(0 .. count-1) --
 * by size (longest-processing-time, zs_partition), each context's share runs on its own host thread through the
 * host-pointer batch call above, and results land in input order.  No collective and no peer traffic: a zlib
 * stream cannot be split bit-exactly, so the buffer is the unit (DeflateCorpusBenchmark.cs:86-100 compresses
 * independent buffers the same way, one after the other).  Contexts must be distinct; several may name the same
 * device.  Returns ZS_OK or the first failing context's code; per-buffer codes in status[i]. */
ZS_API int zs_device_count(void);
/* part_of[i] = context index of buffer i; deterministic (ties: earlier buffer first, lower context first). */
ZS_API int zs_partition(const int64_t *sizes, int n, int n_parts, int *part_of);
ZS_API int zs_deflate_batch_multi(zs_ctx *const *ctxs, int n_ctx, int n, const void *const *in, const int64_t *in_len,
                                  void *const *out, const int64_t *out_cap, int64_t *out_len, int *status, int level,
                                  int strategy, int hash_variant);
/* Device-pointer form: in[i] / out[i] live on the GPU of context part_of[i] (the caller places the buffers, e.g. by
 * zs_partition over the sizes, and keeps them resident): no PCIe traffic, each context's share runs on its own host
 * thread through zs_deflate_batch_device.  out_len / status are HOST arrays. */
ZS_API int zs_deflate_batch_multi_device(zs_ctx *const *ctxs, int n_ctx, int n, const void *const *in, const int64_t *in_len,
                                         void *const *out, const int64_t *out_cap, int64_t *out_len, int *status,
                                         const int *part_of, int level, int strategy, int hash_variant);
ZS_API int zs_inflate_batch_multi(zs_ctx *const *ctxs, int n_ctx, int n, const void *const *in, const int64_t *in_len,
                                  void *const *out, const int64_t *out_cap, int64_t *out_len, int *status);
/* ... over device pointers, as zs_deflate_batch_multi_device: stream i and its output live on the GPU of ctxs[part_of[i]]
 * (zs_partition over the decoded sizes gives a balanced part_of). */
ZS_API int zs_inflate_batch_multi_device(zs_ctx *const *ctxs, int n_ctx, int n, const void *const *in, const int64_t *in_len,
                                         void *const *out, const int64_t *out_cap, int64_t *out_len, int *status, const int *part_of);

/* ------------------------------------------------------------------ */
/* PNG scanline filtering on the device (the caller path of the sparse case -- the reference exists
 * for ImageSharp's PNG encoder, readme.md:16-19, which filters every scanline and writes the rows to ZlibOutputStream).
 * pixels: height rows of row_bytes bytes (device pointer); bpp: bytes per complete pixel, 1..8 (PNG specification 9.2);
 * filter: 0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth, 5 adaptive (per row the filter with the smallest sum of absolute
 * values, first one on ties).  out (device pointer): height * (row_bytes + 1) bytes, every row preceded by its filter
 * type -- the IDAT payload before compression, ready for zs_deflate_batch_device.  With hip_stream == NULL the call
 * returns when the rows are written; otherwise it is ordered on that stream. */
ZS_API int zs_png_filter_device(zs_ctx *ctx, const void *pixels, int64_t row_bytes, int64_t height, int bpp, int filter,
                                void *out, void *hip_stream);

/* zs_png_filter_device for n images in one launch: pixels / out are HOST arrays of DEVICE pointers, row_bytes / height /
 * bpp / filter HOST arrays; the rules per image are those above and the bytes those of n single calls (the tie rule of
 * filter 5 included).  n == 0 is ZS_OK; n < 0, a null array, a bad image or more than 2^31 - 1 rows in one call is
 * ZS_STREAM_ERROR.  The call waits for hip_stream once (its descriptors go through the context's staging buffer);
 * with hip_stream == NULL it returns when the rows are written, otherwise the launch is ordered on that stream. */
ZS_API int zs_png_filter_batch_device(zs_ctx *ctx, int n, const void *const *pixels, const int64_t *row_bytes,
                                      const int64_t *height, const int *bpp, const int *filter, void *const *out,
                                      void *hip_stream);

/* Pixels to IDAT payloads, n images a call, nothing leaving HBM: zs_png_filter_batch_device into a buffer the context
 * owns (height * (row_bytes + 1) bytes per image, kept until zs_ctx_destroy), then zs_deflate_writes_batch_device with
 * one Write per rows_per_write rows -- 1: the scanline-by-scanline encoder, 0: one Write per image.  out[i] receives
 * the zlib stream of image i; out_cap / out_len / status / level / strategy / hash_variant as for the deflate call,
 * whose remarks on the literal engine apply (rows_per_write = 1 at levels 1-3). */
ZS_API int zs_png_idat_batch_device(zs_ctx *ctx, int n, const void *const *pixels, const int64_t *row_bytes,
                                    const int64_t *height, const int *bpp, const int *filter, int64_t rows_per_write,
                                    void *const *out, const int64_t *out_cap, int64_t *out_len, int *status, int level,
                                    int strategy, int hash_variant, void *hip_stream);

/* Inverse of zs_png_filter_device: n independent filtered images (what zs_inflate_batch_device leaves for a PNG's
 * IDAT payload, or for one Adam7 pass), each height[i] rows of 1 + row_bytes[i] bytes (filter type 0..4, then the
 * filtered bytes), reconstructed per PNG specification 9.2 into height[i] * row_bytes[i] bytes of pixels.
 * in[i] / out[i]: DEVICE pointers on ctx's GPU, must not overlap.  bpp[i]: bytes per complete pixel, 1..8.
 * row_bytes / height / bpp / status are HOST arrays.  Work is ordered on hip_stream (NULL = the context's stream);
 * the call synchronises that stream once and returns after the results are known, like zs_inflate_batch_device.
 * status[i] (may be NULL): ZS_OK, or ZS_DATA_ERROR when a row's filter-type byte is > 4 (zs_ctx_last_error names the
 * image and the first such row; that image's output is unspecified, the others are unaffected).
 * Returns ZS_OK, the first failing image's code, or ZS_STREAM_ERROR for bad arguments (also: more than 2^31 - 1 rows in
 * one call), or ZS_MEM_ERROR when the call's workspace (16 bytes per row) does not fit the device.
 * zs_ctx_counter(ctx, "png_segments"): the independent runs of rows the last call found -- a run starts at
 * row 0 and at every None or Sub row, and one run is one workgroup's job (KU). */
ZS_API int zs_png_unfilter_batch_device(zs_ctx *ctx, int n, const void *const *in, const int64_t *row_bytes,
                                        const int64_t *height, const int *bpp, void *const *out, int *status,
                                        void *hip_stream);
/* One image: the batch call with n = 1. */
ZS_API int zs_png_unfilter_device(zs_ctx *ctx, const void *in, int64_t row_bytes, int64_t height, int bpp, void *out,
                                  void *hip_stream);

/* Inflated size of a PNG's IDAT payload and, for interlace = 1, the seven passes' row_bytes[7] / rows[7] (0 / 0 for an
 * absent pass; interlace = 0: entry 0 is the image, the rest 0).  -1 for bad arguments.  Pure host code, no GPU needed.
 * bits_per_pixel: 1, 2, 4, 8, 16, 24, 32, 48 or 64 (bit depth times channels); width and height 1 .. 2^31 - 1.  A pass of
 * Adam7 (PNG specification 8.2) that has no pixels is absent from the stream: no rows, no filter bytes.  Either array may
 * be NULL. */
ZS_API int64_t zs_png_idat_layout(int64_t width, int64_t height, int bits_per_pixel, int interlace, int64_t *row_bytes7,
                                  int64_t *rows7);

/* The Adam7 interleave on the device, n images a call.
 * passes[i]: image i's reconstructed passes back to back in pass order (no filter bytes; absent passes absent), device pointer;
 * out[i]: height[i] rows of ceil(width[i] * bits_per_pixel[i] / 8) bytes, device pointer of any alignment, must not overlap
 * passes[i].  At 1, 2 and 4 bits the unused low bits of a row's last byte are written as zero.  Ordered on hip_stream
 * (NULL: the context's, and the call returns when the pixels are written), like zs_png_filter_batch_device: the call waits
 * for the stream once, for its descriptors' upload.  ZS_STREAM_ERROR for bad arguments (as for zs_png_decode_batch_device),
 * ZS_MEM_ERROR when the descriptors do not fit. */
ZS_API int zs_png_adam7_merge_batch_device(zs_ctx *ctx, int n, const void *const *passes, const int64_t *width,
                                           const int64_t *height, const int *bits_per_pixel, void *const *out, void *hip_stream);

/* IDAT payloads to pixels, n images a call, nothing leaving HBM, interlaced or not: zs_inflate_batch_device into a buffer
 * the context owns, zs_png_unfilter_batch_device's kernels over every image -- or every present Adam7 pass -- whose stream
 * decoded to exactly the length zs_png_idat_layout gives, and the interleave of zs_png_adam7_merge_batch_device for the
 * interlaced ones.
 * idat[i] / idat_len[i]: image i's IDAT chunks' data concatenated = one zlib stream (device pointer); out[i]: height rows of
 * ceil(width * bits_per_pixel / 8) bytes of raw PNG scanline data (device pointer, no bit-depth expansion, no palette).
 * status[i] (may be NULL): ZS_OK or ZS_DATA_ERROR; a failing image leaves the others complete, its own out[i] is
 * unspecified.  zs_ctx_last_error names the first failing image: inflate's message ("incorrect data check", ...; where
 * several streams fail in inflate, the message inflate left for the call), "IDAT holds ... the image needs ..." for a
 * stream of the wrong length, or the pass and row whose filter type is above 4.
 * Returns ZS_OK, ZS_DATA_ERROR, ZS_MEM_ERROR (the workspace does not fit) or, before any device work and with status
 * untouched, ZS_STREAM_ERROR: null context, n < 0, null arrays or pointers, width or height below 1, a bits_per_pixel
 * outside the set, interlace other than 0 or 1, a payload above 2 GiB - 1 KiB, more than 2^31 - 1 rows (pass rows counted)
 * in one call.  Work is ordered on hip_stream (NULL: the context's); the call waits for it twice (inflate's results decide
 * what is reconstructed) and returns when the pixels are written.  The context keeps both buffers until zs_ctx_destroy. */
ZS_API int zs_png_decode_batch_device(zs_ctx *ctx, int n, const void *const *idat, const int64_t *idat_len,
                                      const int64_t *width, const int64_t *height, const int *bits_per_pixel,
                                      const int *interlace, void *const *out, int *status, void *hip_stream);

/* ------------------------------------------------------------------ */
/* CRC-32 (IEEE 802.3, reflected polynomial 0xEDB88320) of device-resident bytes: zlib's crc32(seed, buf, len), the pre- and
 * post-inversion included -- seed 0 starts a CRC, a result fed back as the seed continues it.  The checksum that ends every
 * chunk of a PNG file (and a gzip member); the engine's own streams carry Adler-32 (zs_adler32_device).
 * d_buf: DEVICE pointer of any alignment (the kernel reads whole aligned 16-byte words, so up to 15 bytes in front of and
 * behind the span are read and ignored; they lie in the same 16-byte granule as a byte of the span).  len: 0 .. 2 GiB - 1 KiB.
 * _batch: n spans in one launch, whatever their lengths -- every span is cut into tiles of 8 KiB, the tiles of all spans
 * share the launch (KC).  d_buf / len / seed / out are HOST arrays of n entries; seed == NULL: all 0;
 * d_buf[i] may be NULL where len[i] is 0.  n == 0 is ZS_OK.  A null context, n < 0, a null array or pointer, a negative or
 * oversized len: ZS_STREAM_ERROR before any device work.  Work is ordered on hip_stream (NULL: the context's); the call
 * synchronises that stream once and returns when the results are known.  ZS_MEM_ERROR: the descriptors do not fit. */
ZS_API int zs_crc32_device(zs_ctx *ctx, const void *d_buf, int64_t len, uint32_t seed, uint32_t *out, void *hip_stream);
ZS_API int zs_crc32_batch_device(zs_ctx *ctx, int n, const void *const *d_buf, const int64_t *len, const uint32_t *seed,
                                 uint32_t *out, void *hip_stream);

/* Bytes of the PNG file that holds a zlib stream of idat_len bytes cut into IDAT chunks of at most idat_chunk_bytes data bytes
 * (0: one chunk; 1 .. 2^31 - 1 otherwise) and extra_len bytes of caller-supplied chunks: signature, IHDR, the extra chunks,
 * the IDAT chunks, IEND.  Exact for the stream length given; zs_png_file_bound(zs_deflate_bound(height * (row_bytes + 1)),
 * idat_chunk_bytes, extra_len) is always enough room for zs_png_encode_batch_device.  -1 for bad arguments (negative values, a
 * chunk size above 2^31 - 1, one chunk for more than 2^31 - 1 bytes).  Pure host code, no GPU needed. */
ZS_API int64_t zs_png_file_bound(int64_t idat_len, int64_t idat_chunk_bytes, int64_t extra_len);

/* Pixels to complete PNG files, n images a call, nothing leaving HBM: zs_png_idat_batch_device into a buffer the context owns
 * (zs_deflate_bound of the filtered image per image, kept until zs_ctx_destroy), then one framing launch that reads every
 * IDAT chunk's data once -- copying it into place, whatever the alignments of the two, and computing its CRC-32 -- and a
 * small one that writes the chunks' length, type and CRC words.
 * pixels[i]: raw PNG scanline data (device pointer): height[i] rows of ceil(width[i] * bits / 8) bytes, non-interlaced, bits =
 * bit_depth[i] * channels(color_type[i]); only the (color type, bit depth) pairs of PNG specification table 11.1.  The filters
 * take bpp = max(1, bits / 8).  filter / rows_per_write / level / strategy / hash_variant: as for zs_png_idat_batch_device,
 * whose zlib stream the IDAT chunks hold byte for byte.
 * extra (HOST array of HOST pointers, may be NULL; extra[i] may be NULL where extra_len[i] is 0): chunks the caller has
 * framed already (PLTE, tRNS, gAMA, ...), written verbatim between IHDR and the first IDAT; only their length fields are
 * looked at (they must add up to extra_len[i]), not their types, order or CRCs.
 * idat_chunk_bytes: data bytes of an IDAT chunk at most (0: one chunk).
 * out[i] (device pointer, any alignment) receives the file: signature, IHDR (compression 0, filter method 0, interlace 0),
 * extra[i], the IDAT chunks, IEND.  out_len[i]: the file's length; status[i] (may be NULL): ZS_OK, ZS_BUF_ERROR when
 * out_cap[i] is below that length (nothing is written for that image, the others complete), or the deflate call's code.
 * Returns ZS_OK, the first failing image's code, ZS_MEM_ERROR, or -- before any device work, status and out_len untouched --
 * ZS_STREAM_ERROR: null context, n < 0, a null array or pointer, width or height outside 1 .. 2^31 - 1, an illegal color
 * type / bit depth pair, a filter outside 0..5, a filtered image above 2 GiB - 1 KiB, malformed extra chunks, a negative
 * rows_per_write, an idat_chunk_bytes outside 0 .. 2^31 - 1, a level or strategy deflate rejects.
 * Work is ordered on hip_stream (NULL: the context's); the call waits for it twice (the stream lengths decide the layout) and
 * returns when the files are written.  zs_ctx_stage_ms shows the framing as "crc32_frame". */
ZS_API int zs_png_encode_batch_device(zs_ctx *ctx, int n, const void *const *pixels, const int64_t *width, const int64_t *height,
                                      const int *bit_depth, const int *color_type, const int *filter, const void *const *extra,
                                      const int64_t *extra_len, int64_t rows_per_write, int64_t idat_chunk_bytes, void *const *out,
                                      const int64_t *out_cap, int64_t *out_len, int *status, int level, int strategy,
                                      int hash_variant, void *hip_stream);

/* ------------------------------------------------------------------ */
/* Interlaced encoding (Adam7, PNG specification 8.2): the three calls below mirror the decode side.
 *
 * The Adam7 split on the device, n images a call, one launch over the flat list of all pass rows (KS):
 * the exact inverse of zs_png_adam7_merge_batch_device.  pixels[i]: height[i] rows of ceil(width[i] * bits_per_pixel[i] / 8)
 * bytes; passes_out[i] receives the image's present passes back to back in pass order, no filter bytes, absent passes absent:
 * zs_png_idat_layout(width, height, bits, 1, ..) bytes minus one per pass row.  Both are DEVICE pointers of any alignment and
 * must not overlap.  At 1, 2 and 4 bits the unused low bits of a pass row's last byte are written as zero, and the unused
 * bits of a source row's last byte are never read into the output.  Arguments, ordering on hip_stream (the call waits for the
 * stream once, for its descriptors' upload), n == 0, ZS_STREAM_ERROR (also: more than 2^31 - 1 pass rows in one call) and
 * ZS_MEM_ERROR as for the merge call.  zs_ctx_stage_ms shows the launch as "png_split". */
ZS_API int zs_png_adam7_split_batch_device(zs_ctx *ctx, int n, const void *const *pixels, const int64_t *width,
                                           const int64_t *height, const int *bits_per_pixel, void *const *passes_out,
                                           void *hip_stream);

/* Pixels to IDAT payloads, interlaced or not, n images a call, nothing leaving HBM: the encode-side mirror of
 * zs_png_decode_batch_device.  interlace: HOST array of 0 or 1 per image, NULL = all 0.  An image with interlace 0 gets
 * byte for byte the stream of zs_png_idat_batch_device with row_bytes = ceil(width * bits / 8) and bpp = max(1, bits / 8).
 * An image with interlace 1 is split into its passes (into a buffer the context owns, kept until zs_ctx_destroy), every
 * present pass is filtered as an image of its own -- filtering restarts per pass, PNG specification 9.2 -- and the seven
 * filtered passes back to back, zs_png_idat_layout(.., 1, ..) bytes, are the stream's input.  filter[i] 0..5 applies to every
 * pass, the adaptive choice is made per pass row.  rows_per_write counts rows of the stream in stream order -- pass rows for
 * an interlaced image, and a Write may span a pass boundary; 1: the scanline-by-scanline encoder, 0: one Write per image.
 * out / out_cap / out_len / status / level / strategy / hash_variant as for zs_deflate_writes_batch_device, whose remarks on
 * the literal engine apply.  ZS_STREAM_ERROR before any device work, status and out_len untouched: a null context, n < 0,
 * null arrays, a null pixels[i] or out[i], a negative out_cap[i], width or height outside 1 .. 2^31 - 1, a bits_per_pixel
 * outside the set, an interlace other than 0 or 1, a filter outside 0..5, a negative rows_per_write, a filtered image
 * (zs_png_idat_layout) above 2 GiB - 1 KiB, more than 2^31 - 1 rows in one call, pass rows counted. */
ZS_API int zs_png_idat_interlace_batch_device(zs_ctx *ctx, int n, const void *const *pixels, const int64_t *width,
                                              const int64_t *height, const int *bits_per_pixel, const int *interlace,
                                              const int *filter, int64_t rows_per_write, void *const *out,
                                              const int64_t *out_cap, int64_t *out_len, int *status, int level, int strategy,
                                              int hash_variant, void *hip_stream);

/* zs_png_encode_batch_device with IHDR's interlace byte per image (HOST array of 0 or 1, NULL = all 0): the call above, then
 * the framing launch; everything else in the file is the same.  zs_png_file_bound(zs_deflate_bound(zs_png_idat_layout(width,
 * height, bits, interlace, 0, 0)), idat_chunk_bytes, extra_len) is always enough room.  With interlace NULL or all 0 the
 * files are byte for byte those of zs_png_encode_batch_device.  An interlace value other than 0 or 1 is ZS_STREAM_ERROR
 * before any device work, status and out_len untouched, like the other argument errors. */
ZS_API int zs_png_encode_interlace_batch_device(zs_ctx *ctx, int n, const void *const *pixels, const int64_t *width,
                                                const int64_t *height, const int *bit_depth, const int *color_type,
                                                const int *filter, const int *interlace, const void *const *extra,
                                                const int64_t *extra_len, int64_t rows_per_write, int64_t idat_chunk_bytes,
                                                void *const *out, const int64_t *out_cap, int64_t *out_len, int *status,
                                                int level, int strategy, int hash_variant, void *hip_stream);

/* What a PNG file's IHDR and chunk chain say.  bits_per_pixel = bit depth times channels; idat_bytes: the IDAT chunks' data
 * together (the zlib stream); pixel_bytes: height rows of ceil(width * bits_per_pixel / 8) bytes, what the decoder writes (2^63 - 1 where that is more);
 * n_idat: IDAT chunks. */
typedef struct zs_png_info {
    int64_t width, height;
    int bit_depth, color_type, interlace, bits_per_pixel;
    int64_t idat_bytes, pixel_bytes;
    int64_t n_idat;
} zs_png_info;

/* The chunk walk of one file in HOST memory, pure host code, no context and no GPU: ZS_OK and *info, or ZS_DATA_ERROR for a bad
 * signature, a truncated chunk, a missing or late IHDR, an IHDR field outside the specification, no IDAT, IDAT chunks that
 * are not consecutive, a missing IEND, or a wrong CRC in a critical chunk (IHDR, PLTE, IDAT, IEND; checked here on the host).
 * Ancillary chunks are stepped over by their length fields: they are neither verified nor interpreted, here or in
 * zs_png_decode_files_batch.  Bytes behind IEND are ignored.  ZS_STREAM_ERROR: null pointers or a negative len. */
ZS_API int zs_png_file_info(const void *file, int64_t len, zs_png_info *info);

/* PNG files to pixels, n files a call.  file[i] / file_len[i]: whole files in HOST memory.  The host walks every file's chunk
 * chain (as zs_png_file_info, the CRCs aside); the files go to the device in one copy through the context's staging buffer;
 * one CRC-32 launch checks the critical chunks (IHDR, PLTE, IDAT, IEND -- ancillary chunks are neither verified nor
 * interpreted) and gathers every file's IDAT data into a buffer the context owns; zs_png_decode_batch_device's inflate,
 * reconstruction and Adam7 interleave run on that.  out[i] (DEVICE pointer, out_cap[i] bytes): raw scanline data,
 * info.pixel_bytes of it, no bit-depth expansion, no palette.  info (HOST, may be NULL): filled for every file whose chain
 * could be walked.  status[i] (may be NULL): ZS_OK, ZS_BUF_ERROR (out_cap[i] < pixel_bytes), or ZS_DATA_ERROR -- a file fails
 * for itself only, its out[i] is unspecified; zs_ctx_last_error names the first failing file and the reason: the walk's (see
 * zs_png_file_info), "CRC error in <type> chunk at offset <o>", or what zs_png_decode_batch_device reports.
 * Returns ZS_OK, the first failing file's code, ZS_MEM_ERROR, or, before any device work and with status untouched,
 * ZS_STREAM_ERROR: null context, n < 0, null arrays or pointers, a negative length or capacity.  Work is ordered on
 * hip_stream (NULL: the context's); the call waits for it three times.  The context keeps its buffers until zs_ctx_destroy. */
ZS_API int zs_png_decode_files_batch(zs_ctx *ctx, int n, const void *const *file, const int64_t *file_len, void *const *out,
                                     const int64_t *out_cap, zs_png_info *info, int *status, void *hip_stream);

/* ------------------------------------------------------------------ */
/* Raw scanlines to pixels a caller can show: RGBA, 8 or 16 bits a channel, for every legal (colour type, bit depth) pair,
 * PLTE and tRNS applied.  Rows of width * 4 (ZS_PNG_RGBA8: bytes R, G, B, A) or width * 8 bytes (ZS_PNG_RGBA16: four uint16 in
 * host order, R, G, B, A), no padding.  Exact integer arithmetic:
 *   a sample v of depth d to 8 bits: v * 255 / (2^d - 1) below 8 bits, v at 8, (v * 255 + 32895) >> 16 at 16 (the rounding of
 *   libpng's png_set_scale_16, not the high byte); to 16 bits: v * 65535 / (2^d - 1), 16-bit samples read big-endian;
 *   gray: R = G = B; alpha: the scaled alpha sample (types 4, 6), else 0 where the pixel's samples at their original depth
 *   equal the tRNS key's low d bits and the maximum elsewhere (no tRNS: the maximum);
 *   palette: index k gives PLTE entry k with alpha k < trns_len ? tRNS[k] : 255, an index at or beyond the PLTE's entries
 *   gives opaque black; to 16 bits every channel times 257. */
#define ZS_PNG_RGBA8 0
#define ZS_PNG_RGBA16 1

/* The expansion on the device, n images a call, one launch over the flat list of all output rows (KX).
 * in[i]: raw scanlines exactly as the decode calls leave them (DEVICE pointer, any alignment); out[i]: height[i] rows of
 * width[i] * 4 or * 8 bytes (DEVICE pointer aligned to 4 or 8), must not overlap in[i].  in / out / width / height /
 * bit_depth / color_type are HOST arrays of n entries.  plte / trns: HOST arrays of HOST pointers to the chunks' data bytes,
 * plte_entries / trns_len their counts: plte_entries[i] 1 .. 256, required at type 3; trns_len[i] 0 (none), 2 at type 0, 6 at
 * type 2, 1 .. plte_entries[i] at type 3.  Both are ignored at types 4 and 6, plte also at types 0 and 2; any of the four
 * arrays may be NULL when no image needs it (trns_len == NULL: no image has a tRNS).  format: ZS_PNG_RGBA8 or ZS_PNG_RGBA16,
 * one value for the call.
 * Returns ZS_OK, ZS_MEM_ERROR (the descriptors do not fit) or, before any device work, ZS_STREAM_ERROR: null context, n < 0,
 * null arrays or pointers, an illegal (type, depth) pair, width or height outside 1 .. 2^31 - 1, counts outside the rules
 * above, a bad format, an out[i] not aligned to the pixel size, more than 2^31 - 1 rows in one call.  n == 0 is ZS_OK.
 * Ordered on hip_stream (NULL: the context's, and the call returns when the pixels are written); the call waits for the
 * stream once, for its descriptors' upload, like zs_png_adam7_merge_batch_device.  zs_ctx_stage_ms shows the launch as
 * "png_expand". */
ZS_API int zs_png_expand_batch_device(zs_ctx *ctx, int n, const void *const *in, const int64_t *width, const int64_t *height,
                                      const int *bit_depth, const int *color_type, const void *const *plte,
                                      const int *plte_entries, const void *const *trns, const int *trns_len, int format,
                                      void *const *out, void *hip_stream);

/* The colours of one file in HOST memory, pure host code, no context and no GPU: zs_png_file_info's walk and checks, and the
 * data bytes of PLTE (plte768, *plte_entries = bytes / 3; 0: none) and tRNS (trns256, *trns_len; 0: none) as
 * zs_png_expand_batch_device takes them.  ZS_DATA_ERROR for what zs_png_file_info rejects and for: a PLTE whose length is no
 * multiple of 3 or outside 3 .. 768, a second PLTE or tRNS, either of them behind the first IDAT, a type-3 file without a
 * PLTE in front of its IDAT, a tRNS in front of the PLTE of a type-3 file, a tRNS whose length is not 2 (type 0), 6 (type 2)
 * or 1 .. the PLTE's entries (type 3), a tRNS whose CRC is wrong (the chunk is interpreted, so it is verified -- on the host:
 * it holds at most 256 bytes).  A tRNS of a type 4 or 6 file and a PLTE of a type 0 or 4 file are ignored (0 is returned
 * for them).  ZS_STREAM_ERROR: null pointers or a negative len. */
ZS_API int zs_png_file_colors(const void *file, int64_t len, void *plte768, int *plte_entries, void *trns256, int *trns_len);

/* zs_png_decode_files_batch with the expansion behind it: PNG files to RGBA pixels, n files a call.  The host walk also
 * captures PLTE and tRNS (zs_png_file_colors); the same upload, CRC-and-gather launch, inflate, reconstruction and Adam7
 * interleave leave raw scanlines in a buffer the context owns (pixel_bytes per file, each on a 256-byte boundary, kept
 * until zs_ctx_destroy), and one zs_png_expand_batch_device launch takes the files that are whole from there to out[i]:
 * width * height * 4 (ZS_PNG_RGBA8) or * 8 (ZS_PNG_RGBA16) bytes, DEVICE pointer aligned to 4 or 8.  status[i]: ZS_OK,
 * ZS_BUF_ERROR (out_cap[i] below that), or ZS_DATA_ERROR for anything zs_png_decode_files_batch or zs_png_file_colors
 * rejects; a file fails for itself only, and zs_ctx_last_error names the first failing file ("data error: file i: ...").
 * Arguments, return values and ZS_STREAM_ERROR cases as for zs_png_decode_files_batch, plus a bad format and an out[i]
 * that is not aligned.  The call waits for hip_stream once more than that call (the descriptors of the expansion). */
ZS_API int zs_png_decode_files_rgba_batch(zs_ctx *ctx, int n, const void *const *file, const int64_t *file_len, int format,
                                          void *const *out, const int64_t *out_cap, zs_png_info *info, int *status,
                                          void *hip_stream);

/* ------------------------------------------------------------------ */
/* RGBA pixels to raw scanlines, the inverse of the expansion above: what an encoder needs in front of filter, deflate and
 * framing when the caller holds RGBA8 or RGBA16 pixels.  Exact integer arithmetic:
 *   a sample v to depth d, from ZS_PNG_RGBA8: v >> (8 - d) for d <= 8, v * 257 for d = 16; from ZS_PNG_RGBA16: v for d = 16,
 *   and for d <= 8 first v8 = (v * 255 + 32895) >> 16 (the expansion's own rounding), then v8 >> (8 - d).  Both invert the
 *   expansion's scaling on every value the expansion can produce;
 *   16-bit samples are written big-endian; below 8 bits pixels are packed most-significant-bit first, and the unused low
 *   bits of a row's last byte are written as zero;
 *   types 0 and 4 take the R sample as gray (the call is meant for pixels zs_png_survey_batch_device found gray; luminance
 *   weighting is the caller's business); types 4 and 6 write the alpha sample; types 0 and 2 without a tRNS ignore alpha;
 *   types 0 and 2 with a tRNS key (the chunk's bytes, as for the expansion) write the key's low d bits for every pixel whose
 *   alpha is 0, and every other pixel's own samples;
 *   type 3 reduces the pixel to RGBA8 as above and writes the index of the first palette entry equal to it in all four
 *   channels, an entry's alpha being trns[k] for k < trns_len and 255 otherwise; a pixel with no equal entry gets index 0
 *   (an entry at or beyond 2^d has no index at depth d and is not looked at).
 *
 * The pack on the device, n images a call, one launch over the flat list of all output rows (KG).
 * in[i]: height[i] rows of width[i] * 4 (ZS_PNG_RGBA8) or * 8 bytes (ZS_PNG_RGBA16: four host-order uint16), DEVICE pointer
 * aligned to 4 or 8; out[i]: height[i] rows of ceil(width[i] * bits / 8) bytes (DEVICE pointer, any alignment), must not
 * overlap in[i].  The arrays, plte / plte_entries / trns / trns_len and their rules are those of zs_png_expand_batch_device.
 * unmatched (HOST, n entries, may be NULL): unmatched[i] receives the number of pixels of a type-3 image that found no equal
 * entry, 0 for the other types.
 * Returns ZS_OK, ZS_MEM_ERROR (the descriptors do not fit) or, before any device work, ZS_STREAM_ERROR for everything
 * zs_png_expand_batch_device refuses, an in[i] not aligned to the pixel size in place of its out[i].  n == 0 is ZS_OK.
 * Ordered on hip_stream (NULL: the context's, and the call returns when the scanlines are written); the call waits for the
 * stream once, for its descriptors' upload, and a second time, for the counts, only when unmatched is not NULL.
 * zs_ctx_stage_ms shows the launch as "png_pack". */
ZS_API int zs_png_pack_batch_device(zs_ctx *ctx, int n, const void *const *in, const int64_t *width, const int64_t *height,
                                    const int *bit_depth, const int *color_type, const void *const *plte,
                                    const int *plte_entries, const void *const *trns, const int *trns_len, int format,
                                    void *const *out, int64_t *unmatched, void *hip_stream);

/* What an image's pixels allow a lossless encoder to drop. */
typedef struct zs_png_survey {
    int opaque;        /* every alpha is the format's maximum */
    int gray;          /* R == G == B at every pixel (all pixels, whatever their alpha) */
    int low8;          /* RGBA8: 1.  RGBA16: every sample of every pixel is a multiple of 257 */
    int sample_depth;  /* low8: the smallest d of 1, 2, 4, 8 such that every R, G and B, as 8-bit values, is a multiple of
                          255 / (2^d - 1); otherwise 16 */
    int n_colors;      /* low8: distinct RGBA8 values, 1 .. 256, or 257 for "more than 256"; otherwise 257 */
    uint8_t colors[256][4];  /* the n_colors values as R, G, B, A, ascending by (A, R, G, B); zero beyond (all zero at 257) */
} zs_png_survey;

/* The survey on the device, n images a call (KV): in[i] as for zs_png_pack_batch_device, out: HOST
 * array of n results.  Two launches: workgroups over runs of rows that each keep a violation mask and a set of at most 256
 * colours in LDS and write a record of their own, then one workgroup per image that merges the records; no atomics outside
 * LDS, and the host sorts the colours, so the results are the same on every run.
 * Returns ZS_OK, ZS_MEM_ERROR or, before any device work, ZS_STREAM_ERROR: null context, n < 0, null arrays or pointers,
 * width or height outside 1 .. 2^31 - 1, a bad format, an in[i] not aligned to the pixel size, too many rows in one call.
 * n == 0 is ZS_OK.  Ordered on hip_stream (NULL: the context's); the call waits for the stream twice, for the upload and
 * for the results.  zs_ctx_stage_ms shows the two launches as "png_survey". */
ZS_API int zs_png_survey_batch_device(zs_ctx *ctx, int n, const void *const *in, const int64_t *width, const int64_t *height,
                                      int format, zs_png_survey *out, void *hip_stream);

/* The (colour type, bit depth) pair for a survey, pure host code, no context and no GPU:
 *   !low8: (0,16) if gray and opaque, (4,16) if gray, (2,16) if opaque, else (6,16);
 *   low8: the base is (0, sample_depth) if gray and opaque, (4,8) if gray, (2,8) if opaque, else (6,8); with n_colors <= 256
 *   the palette depth p is 1, 2, 4 or 8 for <= 2, <= 4, <= 16 or more colours, and (3, p) is chosen only if p is strictly
 *   less than the base's bits per pixel -- a tie keeps the base, which needs no PLTE.
 * The rule compares bits per pixel.  It does not promise the smallest file: for a tiny image the PLTE chunk can cost more
 * than the palette saves.  It never chooses a tRNS colour key.  ZS_STREAM_ERROR: null pointers, or a survey whose
 * sample_depth or n_colors is outside its values. */
ZS_API int zs_png_choose_format(const zs_png_survey *s, int *color_type, int *bit_depth);

/* RGBA pixels to complete PNG files, n images a call: the survey, zs_png_choose_format per image, for palette images a PLTE
 * of the survey's colours in its order and a tRNS of their alphas up to the last one below 255 (none when all are 255),
 * both framed on the host, the pack into a buffer the context owns (kept until zs_ctx_destroy), then
 * zs_png_encode_interlace_batch_device on that buffer with extra[i] + PLTE + tRNS as the extra chunks -- the files are byte
 * for byte that call's.  pixels[i] / format as in[i] / format of zs_png_pack_batch_device; every other argument as for
 * zs_png_encode_interlace_batch_device.  color_type_out / bit_depth_out (HOST, n entries, may be NULL): the chosen pairs.
 * A caller's chunks that must follow PLTE (bKGD, hIST) are not supported: extra[i] goes in front of it.
 * zs_png_file_bound(zs_deflate_bound(zs_png_idat_layout(width, height, 32 or 64, interlace, 0, 0)), idat_chunk_bytes,
 * extra_len + 1048) is always enough room; a short out_cap[i] is ZS_BUF_ERROR for that image only.  Argument errors are
 * ZS_STREAM_ERROR before any device work, status and out_len untouched; the 2 GiB - 1 KiB limit of a filtered image is held
 * against the pixels at 32 or 64 bits, whatever pair would be chosen. */
ZS_API int zs_png_encode_rgba_batch_device(zs_ctx *ctx, int n, const void *const *pixels, const int64_t *width,
                                           const int64_t *height, int format, const int *filter, const int *interlace,
                                           const void *const *extra, const int64_t *extra_len, int64_t rows_per_write,
                                           int64_t idat_chunk_bytes, void *const *out, const int64_t *out_cap, int64_t *out_len,
                                           int *status, int *color_type_out, int *bit_depth_out, int level, int strategy,
                                           int hash_variant, void *hip_stream);

/* ------------------------------------------------------------------ */
/* Animated PNG (APNG specification 1.0).  One play's canvases are produced: delays and n_plays are reported, not
 * interpreted -- timing and looping are the viewer's business.  Frames share IHDR's colour type, bit depth and interlace
 * method, and the file's PLTE / tRNS. */
typedef struct zs_png_frame {
    int64_t x, y, width, height;  /* the frame's region of the canvas */
    int delay_num, delay_den;     /* as in the file, not interpreted (0 is legal) */
    int dispose_op, blend_op;     /* 0 NONE, 1 BACKGROUND, 2 PREVIOUS; 0 SOURCE, 1 OVER */
    int64_t data_bytes, n_chunks; /* the frame's zlib stream: IDAT data, or fdAT data without the sequence numbers */
} zs_png_frame;
typedef struct zs_png_anim {
    zs_png_info png;       /* what zs_png_file_info gives */
    int animated;          /* the file has an acTL */
    int n_frames, n_plays; /* acTL's; a file without acTL: 1 and 0 */
    int default_is_frame;  /* an fcTL stands in front of IDAT (always 1 for a file without acTL) */
} zs_png_anim;

/* The animation of one file in HOST memory, pure host code, no context and no GPU: zs_png_file_info's and
 * zs_png_file_colors' walks and checks, then the walk over acTL, fcTL and fdAT.  frames (may be NULL with frames_cap 0)
 * receives the first min(frames_cap, n_frames) frames.  A file without an acTL is an animation of one frame: the whole canvas,
 * dispose NONE, blend SOURCE, its data the IDAT stream; any fcTL / fdAT it holds is stepped over like other ancillary chunks.
 * ZS_BUF_ERROR: frames_cap < n_frames (*anim is filled all the same).  ZS_DATA_ERROR for what the two other walks reject and for:
 *   acTL: a second one, a length other than 8, one behind the first IDAT, num_frames 0 or above 2^31 - 1;
 *   fcTL: a length other than 26, a sequence number that is not the next one (fcTL and fdAT share one counter from 0), more
 *     than one in front of IDAT, one in front of IDAT that is not exactly the canvas at (0, 0), two in a row with no frame data
 *     between them or a last one with none, width or height 0, x + width or y + height beyond the canvas, dispose above 2,
 *     blend above 1;
 *   fdAT: one shorter than 4 bytes, one with the wrong sequence number, one in front of IDAT, one with no fcTL since IDAT;
 *   a number of fcTLs other than num_frames; a wrong CRC in acTL or fcTL (they are interpreted, so they are verified here).
 * fdAT CRCs are not read here: zs_png_decode_anim_batch checks them on the device with the IDAT ones.  Other chunks between a
 * frame's fdATs are stepped over.  ZS_STREAM_ERROR: null file or anim, a negative len or frames_cap, frames NULL with
 * frames_cap > 0. */
ZS_API int zs_png_anim_info(const void *file, int64_t len, zs_png_anim *anim, zs_png_frame *frames, int frames_cap);

/* Frames to canvases on the device, n animations a call, one launch over the flat list of all canvas rows (DESIGN.md
 * section 4, KM).  frame_px[i][f]: DEVICE pointer to frame f's own pixels, frames[i][f].height rows of frames[i][f].width * 4
 * (ZS_PNG_RGBA8) or * 8 (ZS_PNG_RGBA16) bytes as zs_png_expand_batch_device writes them, aligned to 4 or 8.  out[i]: DEVICE
 * pointer, aligned likewise, to n_frames[i] canvases of height[i] * width[i] * 4 or * 8 bytes back to back; canvas f is what a
 * viewer shows while frame f is up.  frame_px, frame_px[i], frames, frames[i], n_frames, width, height and out are HOST
 * arrays; of a frame only x, y, width, height, dispose_op and blend_op are read.  Exact integer arithmetic:
 *   the canvas starts as transparent black; blend SOURCE: the region takes the frame's pixels; blend OVER, per pixel, with
 *   M = 255 or 65535, foreground (f, fa), canvas (b, ba): fa == 0 leaves the canvas alone, fa == M or ba == 0 copies the
 *   frame's pixel, otherwise u = fa * M, v = (M - fa) * ba, al = u + v, every colour channel becomes (f * u + b * v) / al and
 *   alpha al / M, both floor divisions -- the arithmetic of the APNG specification's sample code;
 *   dispose, after canvas f is written: NONE keeps the canvas, BACKGROUND sets the region to transparent black, PREVIOUS
 *   puts back what the region held before frame f was drawn and acts as BACKGROUND on frame 0.
 * Returns ZS_OK, ZS_MEM_ERROR (the descriptors do not fit) or, before any device work, ZS_STREAM_ERROR: null context, n < 0,
 * null arrays or pointers, n_frames[i] < 1, width or height outside 1 .. 2^31 - 1, a region outside the canvas, a dispose or
 * blend value outside the above, a bad format, a misaligned pointer, more than 2^31 - 1 canvas rows (a row counted once per
 * 1024 bytes of it) or frames in one call.
 * n == 0 is ZS_OK.  Ordered on hip_stream (NULL: the context's, and the call returns when the canvases are written); the
 * call waits for the stream once, for its descriptors' upload, like zs_png_expand_batch_device.  zs_ctx_stage_ms shows the
 * launch as "png_compose". */
ZS_API int zs_png_compose_batch_device(zs_ctx *ctx, int n, const void *const *const *frame_px, const zs_png_frame *const *frames,
                                       const int *n_frames, const int64_t *width, const int64_t *height, int format,
                                       void *const *out, void *hip_stream);

/* PNG files, animated or not, to composed canvases, n files a call.  The host walks of zs_png_anim_info (the CRCs of the
 * critical chunks and of fdAT aside), one upload, one CRC-32 launch that checks the critical chunks and every frame's fdAT
 * chunks and gathers each frame's data -- IDAT data, or fdAT data without the sequence numbers -- into a buffer the context
 * owns; one zs_png_decode_batch_device call over all frames of all files as images of their own size; one
 * zs_png_expand_batch_device launch into a second buffer of the context; the compose launch into out[i]: anim[i].n_frames
 * canvases of width * height * 4 (ZS_PNG_RGBA8) or * 8 (ZS_PNG_RGBA16) bytes, DEVICE pointer aligned to 4 or 8.  A default
 * image that is not a frame is not decoded.  A still file gives one canvas: zs_png_decode_files_rgba_batch's pixels.
 * anim (HOST, may be NULL): filled for every file whose chain could be walked.  status[i] (may be NULL): ZS_OK, ZS_BUF_ERROR
 * (out_cap[i] below the canvases' size) or ZS_DATA_ERROR; a file fails for itself only -- for its chunk chain, any CRC, any
 * frame's stream or a frame's length -- and none of its canvases is then specified; zs_ctx_last_error names the first failing
 * file, the frame and the reason ("data error: file i: frame f: ...").  Arguments, return values, ZS_STREAM_ERROR cases and
 * waits as for zs_png_decode_files_rgba_batch, one wait more for the descriptors of the compose launch.  zs_ctx_stage_ms
 * shows "crc32_frame", "png_expand" and "png_compose". */
ZS_API int zs_png_decode_anim_batch(zs_ctx *ctx, int n, const void *const *file, const int64_t *file_len, int format,
                                    void *const *out, const int64_t *out_cap, zs_png_anim *anim, int *status, void *hip_stream);

/* The frame diff, n animations a call (KD): what an APNG writer needs to know about canvases that lie
 * in device memory.  canvases[i]: DEVICE pointer to n_frames[i] canvases of height[i] * width[i] * 4 (ZS_PNG_RGBA8) or * 8
 * (ZS_PNG_RGBA16) bytes back to back, aligned to 4 or 8 -- the layout zs_png_compose_batch_device writes into out[i].
 * frames_out[i]: HOST array of n_frames[i] entries, of which x, y, width and height are written and dispose_op / blend_op
 * set to 0 / 0 (NONE / SOURCE); the delay and data fields are left alone.  The rule is exact:
 *   frame 0 is the whole canvas; frame f >= 1 is the smallest rectangle that holds every pixel whose bytes in canvas f differ
 *   from canvas f - 1 -- all four channels count, a colour change under alpha 0 counts, at RGBA16 the low byte of a sample
 *   counts; where no pixel differs, the 1 x 1 rectangle at (0, 0): APNG has no empty frame.
 * Drawing frame f's rectangle of canvas f with blend SOURCE over canvas f - 1 under dispose NONE gives canvas f byte for byte.
 * Two launches: a wave per 64 groups of 16 bytes of a canvas row carries its groups through the canvases in registers -- every
 * canvas is read once -- and writes one record per frame; one workgroup per (animation, frame) folds the records.  No atomics:
 * the results are the same on every run.  An animation of one frame launches nothing for itself.
 * Returns ZS_OK, ZS_MEM_ERROR (the descriptors or records do not fit) or, before any device work, ZS_STREAM_ERROR: null
 * context, n < 0, null arrays or pointers, n_frames[i] < 1, width or height outside 1 .. 2^31 - 1, a bad format, a misaligned
 * pointer, more than 2^31 - 1 canvas rows (a row counted once per 1024 bytes of it) or frames in one call.  n == 0 is ZS_OK.
 * Ordered on hip_stream (NULL: the context's); the call waits for the stream twice, for the upload of its descriptors and for
 * the rectangles.  zs_ctx_stage_ms shows both launches as "png_diff". */
ZS_API int zs_png_diff_batch_device(zs_ctx *ctx, int n, const void *const *canvases, const int *n_frames, const int64_t *width,
                                    const int64_t *height, int format, zs_png_frame *const *frames_out, void *hip_stream);

/* Rectangles of images as tight rows, n a call, one launch over the flat list of all output rows.  in[i]: DEVICE pointer to an
 * image whose rows are in_width[i] * pixel_bytes bytes; the rectangle of width[i] x height[i] pixels at (x[i], y[i]) goes to
 * out[i] (DEVICE) as height[i] rows of width[i] * pixel_bytes bytes.  pixel_bytes is 4 or 8; in[i] and out[i] are aligned to it
 * and do not overlap.  The image's height is not an argument: the caller vouches for y + height.  Arrays are HOST arrays.
 * Errors, ordering and the single wait (for the descriptors' upload) as for zs_png_expand_batch_device; in addition x or y
 * below 0 and x + width > in_width are ZS_STREAM_ERROR.  n == 0 is ZS_OK.  zs_ctx_stage_ms shows the launch as "png_crop". */
ZS_API int zs_png_crop_batch_device(zs_ctx *ctx, int n, const void *const *in, const int64_t *in_width, const int64_t *x,
                                    const int64_t *y, const int64_t *width, const int64_t *height, int pixel_bytes, void *const *out,
                                    void *hip_stream);

/* Room that zs_png_encode_anim_batch_device never exceeds for one animation, pure host code: every frame taken as the whole
 * canvas at 32 (ZS_PNG_RGBA8) or 64 bits a pixel -- zs_deflate_bound(zs_png_idat_layout(width, height, 32 or 64, interlace, 0,
 * 0)) per frame, 12 bytes per IDAT and 16 per fdAT chunk of at most idat_chunk_bytes stream bytes (0: one chunk), 38 per
 * fcTL, 20 for acTL, 1048 for PLTE + tRNS, extra_len, signature, IHDR and IEND.  For n_frames == 1 it is not below
 * zs_png_file_bound(..., extra_len + 1048) of the still encoder.  -1 for arguments the encoder refuses: width or height
 * outside 1 .. 2^31 - 1, n_frames < 1, a bad format or interlace value, idat_chunk_bytes outside 0 .. 2^31 - 1, extra_len < 0,
 * a canvas above 2 GiB - 1 KiB once filtered, one chunk asked for a stream it cannot hold. */
ZS_API int64_t zs_png_anim_bound(int64_t width, int64_t height, int n_frames, int format, int interlace, int64_t idat_chunk_bytes,
                                 int64_t extra_len);

/* Canvases to animated PNG files, n animations a call: the inverse of zs_png_decode_anim_batch, which returns the canvases
 * byte for byte.  canvases, n_frames, width, height, format: as for zs_png_diff_batch_device.  delay_num / delay_den: HOST
 * arrays of HOST arrays, n_frames[i] values 0 .. 65535 each, written into the fcTLs as given.  n_plays (HOST): 0 .. 2^31 - 1
 * per animation.  filter, interlace (may be NULL), extra, extra_len, rows_per_write, idat_chunk_bytes, out, out_cap, out_len,
 * status, color_type_out, bit_depth_out, level, strategy, hash_variant: as for zs_png_encode_rgba_batch_device, per animation;
 * filter[i] and interlace[i] apply to each of its frames, and a frame is interlaced as an image of its region's size.
 * frames_out (may be NULL): HOST array of HOST arrays, n_frames[i] entries that receive what zs_png_anim_info would report for
 * the file: region, the caller's delays, dispose 0, blend 0, data_bytes, n_chunks.  Steps:
 *   the survey over an animation's canvases as ONE image of n_frames * height rows, and zs_png_choose_format once per
 *   animation: all frames share IHDR's pair and the file's PLTE / tRNS, framed on the host as by the still encoder;
 *   the diff (above); the crop of every frame f >= 1 into a buffer the context owns (frame 0, and a region as wide as the
 *   canvas, are read in place); the pack over all frames of all animations as images of their regions' sizes with the
 *   animation's palette -- it holds every colour of every canvas, so a pixel without an entry is an internal error, reported
 *   as ZS_STREAM_ERROR for that animation with a message that says so; zs_png_idat_interlace_batch_device over all frames;
 *   the layout: signature, IHDR (the canvas), extra[i], PLTE, tRNS, acTL (n_frames, n_plays), fcTL 0 (the whole canvas at
 *   (0, 0)), frame 0's IDAT chunks, then per frame an fcTL and its fdAT chunks of at most idat_chunk_bytes stream bytes, fcTL
 *   and fdAT numbered by one counter from 0, IEND.  Every fcTL has dispose NONE and blend SOURCE.  acTL, fcTL and IEND are
 *   host bytes with host CRCs; IDAT and fdAT are framed on the device in one CRC-32 launch.
 * n_frames[i] == 1 writes no acTL and no fcTL: the file is zs_png_encode_rgba_batch_device's for the one canvas, byte for
 * byte.  zs_png_anim_bound is always enough room; a short out_cap[i] is ZS_BUF_ERROR for that animation only (out_len[i] says
 * what it needs, nothing is written for it); a failing deflate costs its animation only.  Argument errors are
 * ZS_STREAM_ERROR before any device work, status and out_len untouched: those of zs_png_diff_batch_device and
 * zs_png_encode_rgba_batch_device, a delay outside 0 .. 65535, a negative n_plays, n_frames * height above 2^31 - 1, a canvas
 * above 2 GiB - 1 KiB once filtered at 32 or 64 bits.  Waits: those of zs_png_encode_rgba_batch_device on the frames, and
 * three more -- two for the diff, one for the crop's descriptors (none where no region is narrower than its canvas) -- and
 * one for the pack's counts where an animation has a palette.  zs_ctx_stage_ms shows "png_survey", "png_diff", "png_crop",
 * "png_pack", "crc32_frame" and the deflate stages.
 * Not done: blend OVER or dispose BACKGROUND / PREVIOUS chosen to shrink files, merging equal
 * consecutive frames into one longer delay, a default image that is not a frame, a tRNS colour key, anything lossy. */
ZS_API int zs_png_encode_anim_batch_device(zs_ctx *ctx, int n, const void *const *canvases, const int *n_frames,
                                           const int64_t *width, const int64_t *height, int format, const int *const *delay_num,
                                           const int *const *delay_den, const int *n_plays, const int *filter, const int *interlace,
                                           const void *const *extra, const int64_t *extra_len, int64_t rows_per_write,
                                           int64_t idat_chunk_bytes, void *const *out, const int64_t *out_cap, int64_t *out_len,
                                           int *status, zs_png_frame *const *frames_out, int *color_type_out, int *bit_depth_out,
                                           int level, int strategy, int hash_variant, void *hip_stream);

/* Stage timing of the last *_batch_device call, measured with hipEvents on
 * the stream the kernels ran on.  Enable before the call. */
/* Counters of a context for tests and measurements (-1: no such counter): "fast_rounds" -- rounds the last call's DeflateFast took
 * over its chunks (0: one workgroup per stream); "fast_fallbacks", "round_runs", "cut_rounds", "lit_fallbacks" -- batches that took
 * one of the slower paths since the context was made; "lit_engine_bytes" -- input bytes the one-wave literal engine parsed
 * beyond the streams' last 261 (a call that runs its batch again counts the plan it ends with); "spec_streams", "spec_fallbacks", "spec_wrong_chunks" -- the last deflate call's speculative
 * chunk walk (levels 4-9): streams that tried it, those of them that took the transfer maps after all, chunks whose guessed
 * entry was wrong; "spec_periodic" -- those of the fallbacks that were never walked (periodic by the match kernel's count);
 * "inf_lane_streams" -- streams of the last inflate call whose chain had blocks for the lane decoder (blocks with checkpoints and
 * no tokens: under 4 bits per symbol, or no room for the token buffers); "inf_wave_streams" -- streams of the last inflate call
 * at or above the block-parallel minimum (1 KiB) that the block-parallel pass could not finish and handed to the one-wave decoder
 * (a chain that does not close, a table or list that overflows, a block that reports failure; streams below the minimum go to
 * that decoder without being counted); "plan_reused" -- 1 if the last deflate call had the shape of the one before (stream
 * count, lengths, capacities, level, strategy, hash variant, Write lists) and took its plan instead of planning, 0 if it planned. */
ZS_API int64_t zs_ctx_counter(const zs_ctx *ctx, const char *name);
/* (A test hook, not part of the product's surface: declared only where ZS_TESTING is defined.)
 * For the tests: what the parse stage of the last deflate call left for its first stream, copied from the device -- "state"
 * (int32 x 6: tail_p, tail_kind, tail_pend, k_done, preins, body_syms), "blk_end" / "blk_top" (int32 per finished block of the
 * body), "symbase" (uint32 per 2048-position chunk, the map path) or "spec_base" (uint32 per chunk of the speculative grid).
 * Returns the bytes written, -1 for an unknown name or too small a buffer. */
#if defined(ZS_TESTING) || defined(ZS_BUILDING_LIBRARY)
ZS_API int64_t zs_ctx_debug_read(zs_ctx *ctx, const char *name, void *out, int64_t cap);
#endif
ZS_API void zs_ctx_set_profiling(zs_ctx *ctx, int enable);
ZS_API int zs_ctx_stage_count(const zs_ctx *ctx);
ZS_API const char *zs_ctx_stage_name(const zs_ctx *ctx, int stage);
ZS_API double zs_ctx_stage_ms(const zs_ctx *ctx, int stage);

/* ------------------------------------------------------------------ */
/* z_stream-shaped streaming interface: what ZLibStream.Deflate(flush) binds to.
 *
 * zs_deflate_init  <- Deflate..ctor (Deflate.cs:228-310): level -1..9,
 *   strategy 0..4, window_bits +-9..15 (negative = no zlib header/trailer),
 *   mem_level 1..9.  Argument errors return NULL (the reference throws
 *   ArgumentOutOfRangeException).
 * zs_deflate       <- Deflate.Compress (Deflate.cs:436-636).  The cursor fields
 *   of ZLibStream (ZlibStream.cs:34-94) are passed explicitly: *avail_in /
 *   *avail_out are decremented, *total_in / *total_out advanced, *adler
 *   updated.  Input is copied during the call.  NoFlush Writes are buffered
 *   and a stream that never flushes is compressed by the bulk pipeline when
 *   ZS_FINISH arrives, after which output is handed out avail_out bytes at a
 *   time exactly like Flush_pending (Deflate.cs:828-854).
 *   ZS_PARTIAL_FLUSH / ZS_SYNC_FLUSH / ZS_FULL_FLUSH (Deflate.cs:583-613) run the
 *   engine at that call and deliver everything up to and including the flush
 *   marker, so the reader can decode what has been written so far; from then on
 *   the stream is incremental (the engine is kept suspended in device memory,
 *   consumed input is dropped); at levels 4-9 the runs behind a flush are the
 *   bulk pipeline's again, started at the flush on the suspended engine's hash
 *   chains, so NoFlush Writes behind a flush wait for the next flush or Finish
 *   like those in front of the first.  A NoFlush stream with more than 1 GiB buffered
 *   becomes incremental too: a stream has no length limit (a single call takes
 *   up to 2 GiB - 1 KiB; 2 GiB - 65 KiB on a stream that has become incremental, whose run keeps 64 KiB of history).  The bytes are the reference's for a caller that runs
 *   ZlibOutputStream.WriteCore's loop (ZlibOutputStream.cs:125-168: a fresh
 *   output chunk of the same size for every call -- the size is taken from the
 *   first call): block end + Tr_align / empty stored block after every flushed
 *   Write, FullFlush forgetting the hash heads, and the extra empty blocks of
 *   flushes that fill the chunk exactly.
 * zs_deflate_end   <- Deflate.Dispose.
 * zs_last_message  <- ZLibStream.Message. */
typedef struct zs_deflate_stream zs_deflate_stream;

ZS_API zs_deflate_stream *zs_deflate_init(zs_ctx *ctx, int level, int strategy, int window_bits, int mem_level,
                                          int hash_variant);
ZS_API int zs_deflate(zs_deflate_stream *s, const uint8_t *next_in, int32_t *avail_in, uint8_t *next_out,
                      int32_t *avail_out, int flush, uint32_t *adler, int64_t *total_in, int64_t *total_out);
ZS_API void zs_deflate_end(zs_deflate_stream *s);
ZS_API const char *zs_last_message(const zs_deflate_stream *s);

/* zs_inflate_init <- Inflate..ctor (Inflate.cs:76-96); only window_bits 15 (zlib-wrapped) runs on the device: NULL otherwise.
 * zs_inflate      <- Inflate.Decompress (Inflate.cs:103-357) as ZLibStream.Inflate(FlushMode) calls it
 *   (ZlibStream.cs:119-122), driven by ZlibInputStream.ReadCore (ZlibInputStream.cs:133-186).  Same cursor convention as
 *   zs_deflate.  Calls that bring input return ZS_OK after taking it.  A whole stream is decoded by the block-parallel
 *   decoder at the call whose input completes it -- the end (final block + Adler-32 trailer, Inflate.cs:292-357) is looked
 *   for in what has been buffered each time the buffered bytes have quadrupled, from 1 MiB on.  A call with *avail_in == 0
 *   (the reader has run out of input for now: ZlibInputStream.ReadCore behind a writer's flush) decodes what the bytes so
 *   far hold in complete blocks -- a flush ends on a block boundary (Deflate.cs:583-613), so everything the writer flushed
 *   is delivered -- and the stream goes on piece by piece from there with the next input; so does a stream that is fed 64
 *   MiB without a call for output (bounded host memory for a stream of any length).  A block is complete when its last
 *   bit has arrived; the final block only when the four trailer bytes behind it have, so it is held back until then
 *   (tests/inflate_stream_cases.py states the rule and pins it).  ZS_STREAM_END comes with the last byte.  total_in is the stream's length with its trailer; bytes behind the trailer that the call which met the end
 *   brought are left to the caller (*avail_in), as the managed engine leaves them; bytes behind it from earlier calls
 *   (the end is only looked for now and then) are kept: zs_inflate_surplus.  A call without input that has nothing new to
 *   give is ZS_BUF_ERROR (Inflate.Decompress's "no progress"); corrupt data gives ZS_DATA_ERROR with the reference's
 *   message (zs_inflate_message).
 *   Malformed streams: incomplete code sets are accepted exactly where Huft_build accepts them (a single code of length
 *   1, InfTree.cs:364); one deliberate difference -- a match distance that reaches before the first output byte is
 *   ZS_DATA_ERROR "invalid distance code" here, the managed engine copies from its zeroed window instead
 *   (InfCodes.cs:241,659). */
typedef struct zs_inflate_stream zs_inflate_stream;
ZS_API zs_inflate_stream *zs_inflate_init(zs_ctx *ctx, int window_bits);
ZS_API int zs_inflate(zs_inflate_stream *s, const uint8_t *next_in, int32_t *avail_in, uint8_t *next_out, int32_t *avail_out,
                      int flush, uint32_t *adler, int64_t *total_in, int64_t *total_out);
ZS_API void zs_inflate_end(zs_inflate_stream *s);
ZS_API const char *zs_inflate_message(const zs_inflate_stream *s);
/* Bytes fed behind the stream's trailer by calls before the one that met the stream's end (no counterpart in the reference,
 * whose engine stops at the trailer byte for byte): count, *p -> the bytes (owned by the stream object). */
ZS_API int64_t zs_inflate_surplus(const zs_inflate_stream *s, const uint8_t **p);

/* Adler32.Calculate (Adler32.cs:61-78) on the GPU, for a device-resident
 * buffer; result returned to the host. */
ZS_API int zs_adler32_device(zs_ctx *ctx, const void *d_buf, int64_t len, uint32_t seed, uint32_t *out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
