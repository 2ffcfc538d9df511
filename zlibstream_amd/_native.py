"""ctypes binding of include/zsgpu.h.  Loading fails loudly: there is no CPU
fallback for the compression path."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZS_DEV=1 ZS_LIB=<path>: another build of the same library (the A/B tools under tools/ select a variant this way instead of
# overwriting the product library); without the explicit development flag the in-tree build is the one that loads
LIB_PATH = (os.environ.get("ZS_LIB") if os.environ.get("ZS_DEV") == "1" else None) or os.path.join(_HERE, "libzsgpu.so")

SYMBOLS = [
    "zs_ctx_create", "zs_ctx_destroy", "zs_ctx_last_error", "zs_deflate_bound", "zs_deflate_batch_device",
    "zs_deflate_batch", "zs_ctx_counter", "zs_ctx_debug_read", "zs_ctx_set_profiling", "zs_ctx_stage_count", "zs_ctx_stage_name", "zs_ctx_stage_ms",
    "zs_deflate_init", "zs_deflate", "zs_deflate_end", "zs_last_message", "zs_adler32_device",
    "zs_inflate_batch_device", "zs_inflate_batch", "zs_inflate_init", "zs_inflate", "zs_inflate_end", "zs_inflate_message", "zs_inflate_surplus",
    "zs_device_count", "zs_partition", "zs_deflate_batch_multi", "zs_inflate_batch_multi", "zs_png_filter_device", "zs_deflate_writes_device", "zs_deflate_batch_multi_device", "zs_inflate_batch_multi_device",
    "zs_png_unfilter_batch_device", "zs_png_unfilter_device",
    "zs_deflate_writes_batch_device", "zs_png_filter_batch_device", "zs_png_idat_batch_device",
    "zs_png_idat_layout", "zs_png_adam7_merge_batch_device", "zs_png_decode_batch_device",
    "zs_crc32_device", "zs_crc32_batch_device", "zs_png_file_bound", "zs_png_encode_batch_device", "zs_png_file_info",
    "zs_png_decode_files_batch",
    "zs_png_expand_batch_device", "zs_png_file_colors", "zs_png_decode_files_rgba_batch",
    "zs_png_adam7_split_batch_device", "zs_png_idat_interlace_batch_device", "zs_png_encode_interlace_batch_device",
    "zs_png_pack_batch_device", "zs_png_survey_batch_device", "zs_png_choose_format", "zs_png_encode_rgba_batch_device",
    "zs_png_anim_info", "zs_png_compose_batch_device", "zs_png_decode_anim_batch",
    "zs_png_diff_batch_device", "zs_png_crop_batch_device", "zs_png_anim_bound", "zs_png_encode_anim_batch_device",
    "zs_wrap_bound", "zs_deflate_wrap_batch_device", "zs_inflate_wrap_batch_device", "zs_gzip_file_info", "zs_gzip_decode_files_batch",
    "zs_zip_file_info", "zs_zip_decode_files_batch", "zs_zip_bound", "zs_zip_encode_batch_device",
    "zs_tiff_file_info", "zs_tiff_unpredict_batch_device", "zs_tiff_predict_batch_device", "zs_tiff_decode_files_batch", "zs_tiff_bound",
    "zs_tiff_encode_batch_device",
    "zs_exr_file_info", "zs_exr_unpredict_batch_device", "zs_exr_predict_batch_device", "zs_exr_decode_files_batch", "zs_exr_bound",
    "zs_exr_encode_batch_device",
    "zs_chunk_grid_info", "zs_chunks_decode_batch", "zs_chunks_bound", "zs_chunks_encode_batch_device", "zs_shuffle_batch_device",
    "zs_unshuffle_batch_device",
    "zs_chunks_decode_filters_batch", "zs_chunks_encode_filters_batch_device", "zs_chunks_filters_bound", "zs_fletcher32_batch_device",
    "zs_delta_encode_batch_device", "zs_delta_decode_batch_device",
]


class PngInfo(ctypes.Structure):  # zs_png_info
    _fields_ = [("width", ctypes.c_int64), ("height", ctypes.c_int64), ("bit_depth", ctypes.c_int), ("color_type", ctypes.c_int),
                ("interlace", ctypes.c_int), ("bits_per_pixel", ctypes.c_int), ("idat_bytes", ctypes.c_int64),
                ("pixel_bytes", ctypes.c_int64), ("n_idat", ctypes.c_int64)]


class GzipInfo(ctypes.Structure):  # zs_gzip_info
    _fields_ = [("bgzf", ctypes.c_int), ("xfl", ctypes.c_int), ("os", ctypes.c_int), ("mtime", ctypes.c_uint32),
                ("n_members", ctypes.c_int64), ("name_off", ctypes.c_int64), ("name_len", ctypes.c_int64), ("isize_sum", ctypes.c_int64)]


class ZipInfo(ctypes.Structure):  # zs_zip_info
    _fields_ = [("n_entries", ctypes.c_int64), ("total_len", ctypes.c_int64), ("cd_off", ctypes.c_int64), ("cd_len", ctypes.c_int64),
                ("shift", ctypes.c_int64), ("comment_off", ctypes.c_int64), ("comment_len", ctypes.c_int64), ("zip64", ctypes.c_int)]


class ZipEntry(ctypes.Structure):  # zs_zip_entry
    _fields_ = [("name_off", ctypes.c_int64), ("name_len", ctypes.c_int), ("method", ctypes.c_int), ("flags", ctypes.c_int),
                ("crc32", ctypes.c_uint32), ("comp_len", ctypes.c_int64), ("len", ctypes.c_int64), ("local_off", ctypes.c_int64),
                ("body_off", ctypes.c_int64), ("out_off", ctypes.c_int64), ("dos_time", ctypes.c_uint16), ("dos_date", ctypes.c_uint16),
                ("external_attr", ctypes.c_uint32), ("status", ctypes.c_int)]


class ZipPut(ctypes.Structure):  # zs_zip_put
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_int64), ("name", ctypes.c_char_p), ("name_len", ctypes.c_int),
                ("method", ctypes.c_int), ("utf8", ctypes.c_int), ("dos_time", ctypes.c_uint16), ("dos_date", ctypes.c_uint16),
                ("external_attr", ctypes.c_uint32)]


class TiffInfo(ctypes.Structure):  # zs_tiff_info
    _fields_ = [("n_pages", ctypes.c_int64), ("big_endian", ctypes.c_int), ("bigtiff", ctypes.c_int), ("width", ctypes.c_int64),
                ("height", ctypes.c_int64), ("bits", ctypes.c_int), ("spp", ctypes.c_int), ("sample_format", ctypes.c_int),
                ("photometric", ctypes.c_int), ("extra_samples", ctypes.c_int), ("extra_kind", ctypes.c_int), ("compression", ctypes.c_int),
                ("predictor", ctypes.c_int), ("planar", ctypes.c_int), ("orientation", ctypes.c_int), ("tiled", ctypes.c_int),
                ("pad", ctypes.c_int), ("chunk_w", ctypes.c_int64), ("chunk_h", ctypes.c_int64), ("n_chunks", ctypes.c_int64),
                ("row_bytes", ctypes.c_int64), ("out_len", ctypes.c_int64)]


class TiffChunk(ctypes.Structure):  # zs_tiff_chunk
    _fields_ = [("off", ctypes.c_int64), ("comp_len", ctypes.c_int64), ("x", ctypes.c_int64), ("y", ctypes.c_int64), ("w", ctypes.c_int64),
                ("h", ctypes.c_int64), ("status", ctypes.c_int), ("pad", ctypes.c_int)]


class TiffPut(ctypes.Structure):  # zs_tiff_put
    _fields_ = [("pixels", ctypes.c_void_p), ("width", ctypes.c_int64), ("height", ctypes.c_int64), ("bits", ctypes.c_int), ("spp", ctypes.c_int),
                ("sample_format", ctypes.c_int), ("photometric", ctypes.c_int), ("extra_samples", ctypes.c_int), ("extra_kind", ctypes.c_int),
                ("predictor", ctypes.c_int), ("pad", ctypes.c_int), ("tile_width", ctypes.c_int64), ("tile_height", ctypes.c_int64),
                ("rows_per_strip", ctypes.c_int64)]


class ExrInfo(ctypes.Structure):  # zs_exr_info
    _fields_ = [("data_window", ctypes.c_int32 * 4), ("display_window", ctypes.c_int32 * 4), ("width", ctypes.c_int64), ("height", ctypes.c_int64),
                ("n_channels", ctypes.c_int), ("compression", ctypes.c_int), ("line_order", ctypes.c_int), ("tiled", ctypes.c_int),
                ("has_display_window", ctypes.c_int), ("long_names", ctypes.c_int), ("tile_w", ctypes.c_int64), ("tile_h", ctypes.c_int64),
                ("lines_per_chunk", ctypes.c_int64), ("n_chunks", ctypes.c_int64), ("out_len", ctypes.c_int64)]


class ExrChannel(ctypes.Structure):  # zs_exr_channel
    _fields_ = [("name", ctypes.c_char * 256), ("type", ctypes.c_int), ("sample_bytes", ctypes.c_int), ("plane_off", ctypes.c_int64)]


class ExrChunk(ctypes.Structure):  # zs_exr_chunk
    _fields_ = [("off", ctypes.c_int64), ("data_len", ctypes.c_int64), ("raw_len", ctypes.c_int64), ("x", ctypes.c_int64), ("y", ctypes.c_int64),
                ("w", ctypes.c_int64), ("h", ctypes.c_int64), ("status", ctypes.c_int), ("pad", ctypes.c_int)]


class ExrPut(ctypes.Structure):  # zs_exr_put
    _fields_ = [("planes", ctypes.c_void_p), ("width", ctypes.c_int64), ("height", ctypes.c_int64), ("x_min", ctypes.c_int32), ("y_min", ctypes.c_int32),
                ("n_channels", ctypes.c_int), ("compression", ctypes.c_int), ("names", ctypes.POINTER(ctypes.c_char_p)),
                ("types", ctypes.POINTER(ctypes.c_int)), ("extra", ctypes.c_char_p), ("extra_len", ctypes.c_int64)]


class ChunkGrid(ctypes.Structure):  # zs_chunk_grid
    _fields_ = [("rank", ctypes.c_int), ("elem_size", ctypes.c_int), ("shape", ctypes.c_int64 * 8), ("chunk", ctypes.c_int64 * 8),
                ("shuffle", ctypes.c_int), ("wrap", ctypes.c_int), ("fill", ctypes.c_uint8 * 16)]


class ChunkFilters(ctypes.Structure):  # zs_chunk_filters
    _fields_ = [("delta", ctypes.c_int), ("byte_order", ctypes.c_int), ("fletcher32", ctypes.c_int), ("reserved", ctypes.c_int)]


class ChunkRef(ctypes.Structure):  # zs_chunk_ref
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_int64), ("flags", ctypes.c_int)]


class PngSurvey(ctypes.Structure):  # zs_png_survey
    _fields_ = [("opaque", ctypes.c_int), ("gray", ctypes.c_int), ("low8", ctypes.c_int), ("sample_depth", ctypes.c_int),
                ("n_colors", ctypes.c_int), ("colors", ctypes.c_uint8 * 4 * 256)]


class PngFrame(ctypes.Structure):  # zs_png_frame
    _fields_ = [("x", ctypes.c_int64), ("y", ctypes.c_int64), ("width", ctypes.c_int64), ("height", ctypes.c_int64),
                ("delay_num", ctypes.c_int), ("delay_den", ctypes.c_int), ("dispose_op", ctypes.c_int), ("blend_op", ctypes.c_int),
                ("data_bytes", ctypes.c_int64), ("n_chunks", ctypes.c_int64)]


class PngAnim(ctypes.Structure):  # zs_png_anim
    _fields_ = [("png", PngInfo), ("animated", ctypes.c_int), ("n_frames", ctypes.c_int), ("n_plays", ctypes.c_int),
                ("default_is_frame", ctypes.c_int)]


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64.so.7; the loader shares one HIP runtime between
    # torch and this library only when torch's copy is mapped first (same SONAME).
    import sys
    if "torch" not in sys.modules and os.environ.get("ZS_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "zlibstream_amd/libzsgpu.so is missing: build it with `python -m zlibstream_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    P = ctypes.POINTER
    L.zs_ctx_create.restype = i32
    L.zs_ctx_create.argtypes = [i32, P(vp)]
    L.zs_ctx_destroy.restype = None
    L.zs_ctx_destroy.argtypes = [vp]
    L.zs_ctx_last_error.restype = ctypes.c_char_p
    L.zs_ctx_last_error.argtypes = [vp]
    L.zs_deflate_bound.restype = i64
    L.zs_deflate_bound.argtypes = [i64]
    batch_args = [vp, i32, P(vp), P(i64), P(vp), P(i64), P(i64), P(i32), i32, i32, i32]
    L.zs_deflate_batch_device.restype = i32
    L.zs_deflate_batch_device.argtypes = batch_args + [vp]
    L.zs_deflate_batch.restype = i32
    L.zs_deflate_batch.argtypes = batch_args
    if hasattr(L, "zs_deflate_writes_device"):  # (an older build selected with ZS_LIB for an A/B run may lack it)
        L.zs_deflate_writes_device.restype = i32
        L.zs_deflate_writes_device.argtypes = [vp, vp, i64, P(i64), i64, vp, i64, P(i64), i32, i32, i32, vp]
    inf_args = [vp, i32, P(vp), P(i64), P(vp), P(i64), P(i64), P(i32)]
    L.zs_inflate_batch_device.restype = i32
    L.zs_inflate_batch_device.argtypes = inf_args + [vp]
    L.zs_inflate_batch.restype = i32
    L.zs_inflate_batch.argtypes = inf_args
    L.zs_ctx_counter.restype = i64
    L.zs_ctx_counter.argtypes = [vp, ctypes.c_char_p]
    if hasattr(L, "zs_ctx_debug_read"):  # (an older build selected with ZS_LIB may lack it)
        L.zs_ctx_debug_read.restype = i64
        L.zs_ctx_debug_read.argtypes = [vp, ctypes.c_char_p, vp, i64]
    L.zs_ctx_set_profiling.restype = None
    L.zs_ctx_set_profiling.argtypes = [vp, i32]
    L.zs_ctx_stage_count.restype = i32
    L.zs_ctx_stage_count.argtypes = [vp]
    L.zs_ctx_stage_name.restype = ctypes.c_char_p
    L.zs_ctx_stage_name.argtypes = [vp, i32]
    L.zs_ctx_stage_ms.restype = ctypes.c_double
    L.zs_ctx_stage_ms.argtypes = [vp, i32]
    L.zs_deflate_init.restype = vp
    L.zs_deflate_init.argtypes = [vp, i32, i32, i32, i32, i32]
    L.zs_deflate.restype = i32
    L.zs_deflate.argtypes = [vp, vp, P(ctypes.c_int32), vp, P(ctypes.c_int32), i32, P(ctypes.c_uint32), P(i64), P(i64)]
    L.zs_deflate_end.restype = None
    L.zs_deflate_end.argtypes = [vp]
    L.zs_last_message.restype = ctypes.c_char_p
    L.zs_last_message.argtypes = [vp]
    L.zs_inflate_init.restype = vp
    L.zs_inflate_init.argtypes = [vp, i32]
    L.zs_inflate.restype = i32
    L.zs_inflate.argtypes = [vp, vp, P(ctypes.c_int32), vp, P(ctypes.c_int32), i32, P(ctypes.c_uint32), P(i64), P(i64)]
    L.zs_inflate_end.restype = None
    L.zs_inflate_end.argtypes = [vp]
    L.zs_inflate_message.restype = ctypes.c_char_p
    L.zs_inflate_message.argtypes = [vp]
    L.zs_inflate_surplus.restype = i64
    L.zs_inflate_surplus.argtypes = [vp, P(vp)]
    L.zs_adler32_device.restype = i32
    L.zs_adler32_device.argtypes = [vp, vp, i64, ctypes.c_uint32, P(ctypes.c_uint32), vp]
    L.zs_device_count.restype = i32
    L.zs_device_count.argtypes = []
    L.zs_partition.restype = i32
    L.zs_partition.argtypes = [P(i64), i32, i32, P(i32)]
    if hasattr(L, "zs_deflate_batch_multi_device"):
        L.zs_deflate_batch_multi_device.restype = i32
        L.zs_deflate_batch_multi_device.argtypes = [P(vp), i32, i32, P(vp), P(i64), P(vp), P(i64), P(i64), P(i32), P(i32), i32, i32, i32]
    L.zs_deflate_batch_multi.restype = i32
    L.zs_deflate_batch_multi.argtypes = [P(vp), i32, i32, P(vp), P(i64), P(vp), P(i64), P(i64), P(i32), i32, i32, i32]
    L.zs_inflate_batch_multi_device.restype = i32
    L.zs_inflate_batch_multi_device.argtypes = [P(vp), i32, i32, P(vp), P(i64), P(vp), P(i64), P(i64), P(i32), P(i32)]
    L.zs_inflate_batch_multi.restype = i32
    L.zs_inflate_batch_multi.argtypes = [P(vp), i32, i32, P(vp), P(i64), P(vp), P(i64), P(i64), P(i32)]
    L.zs_png_filter_device.restype = i32
    L.zs_png_filter_device.argtypes = [vp, vp, i64, i64, i32, i32, vp, vp]
    L.zs_png_unfilter_batch_device.restype = i32
    L.zs_png_unfilter_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(i32), P(vp), P(i32), vp]
    L.zs_png_unfilter_device.restype = i32
    L.zs_png_unfilter_device.argtypes = [vp, vp, i64, i64, i32, vp, vp]
    if hasattr(L, "zs_deflate_writes_batch_device"):  # (an older build selected with ZS_LIB for an A/B run lacks the batch encoder)
        L.zs_deflate_writes_batch_device.restype = i32
        L.zs_deflate_writes_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(P(i64)), P(i64), P(vp), P(i64), P(i64), P(i32), i32, i32, i32, vp]
        L.zs_png_filter_batch_device.restype = i32
        L.zs_png_filter_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(i32), P(i32), P(vp), vp]
        L.zs_png_idat_batch_device.restype = i32
        L.zs_png_idat_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(i32), P(i32), i64, P(vp), P(i64), P(i64), P(i32), i32, i32, i32, vp]
    if hasattr(L, "zs_png_decode_batch_device"):  # (an older build selected with ZS_LIB for an A/B run lacks the decoder)
        L.zs_png_idat_layout.restype = i64
        L.zs_png_idat_layout.argtypes = [i64, i64, i32, i32, P(i64), P(i64)]
        L.zs_png_adam7_merge_batch_device.restype = i32
        L.zs_png_adam7_merge_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(i32), P(vp), vp]
        L.zs_png_decode_batch_device.restype = i32
        L.zs_png_decode_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(i64), P(i32), P(i32), P(vp), P(i32), vp]
    if hasattr(L, "zs_crc32_batch_device"):  # (an older build selected with ZS_LIB for an A/B run lacks CRC-32 and the file calls)
        u32 = ctypes.c_uint32
        L.zs_crc32_device.restype = i32
        L.zs_crc32_device.argtypes = [vp, vp, i64, u32, P(u32), vp]
        L.zs_crc32_batch_device.restype = i32
        L.zs_crc32_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(u32), P(u32), vp]
        L.zs_png_file_bound.restype = i64
        L.zs_png_file_bound.argtypes = [i64, i64, i64]
        L.zs_png_encode_batch_device.restype = i32
        L.zs_png_encode_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(i32), P(i32), P(i32), P(vp), P(i64), i64, i64, P(vp), P(i64),
                                                 P(i64), P(i32), i32, i32, i32, vp]
        L.zs_png_file_info.restype = i32
        L.zs_png_file_info.argtypes = [vp, i64, P(PngInfo)]
        L.zs_png_decode_files_batch.restype = i32
        L.zs_png_decode_files_batch.argtypes = [vp, i32, P(vp), P(i64), P(vp), P(i64), P(PngInfo), P(i32), vp]
    if hasattr(L, "zs_png_expand_batch_device"):  # (an older build selected with ZS_LIB for an A/B run lacks the expansion to RGBA)
        L.zs_png_expand_batch_device.restype = i32
        L.zs_png_expand_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(i32), P(i32), P(vp), P(i32), P(vp), P(i32), i32, P(vp), vp]
        L.zs_png_file_colors.restype = i32
        L.zs_png_file_colors.argtypes = [vp, i64, vp, P(i32), vp, P(i32)]
        L.zs_png_decode_files_rgba_batch.restype = i32
        L.zs_png_decode_files_rgba_batch.argtypes = [vp, i32, P(vp), P(i64), i32, P(vp), P(i64), P(PngInfo), P(i32), vp]
    if hasattr(L, "zs_png_adam7_split_batch_device"):  # (an older build selected with ZS_LIB for an A/B run lacks the interlaced encoder)
        L.zs_png_adam7_split_batch_device.restype = i32
        L.zs_png_adam7_split_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(i32), P(vp), vp]
        L.zs_png_idat_interlace_batch_device.restype = i32
        L.zs_png_idat_interlace_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(i32), P(i32), P(i32), i64, P(vp), P(i64), P(i64), P(i32),
                                                         i32, i32, i32, vp]
        L.zs_png_encode_interlace_batch_device.restype = i32
        L.zs_png_encode_interlace_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(i32), P(i32), P(i32), P(i32), P(vp), P(i64), i64, i64,
                                                           P(vp), P(i64), P(i64), P(i32), i32, i32, i32, vp]
    if hasattr(L, "zs_png_pack_batch_device"):  # (an older build selected with ZS_LIB for an A/B run lacks the encoder from RGBA)
        L.zs_png_pack_batch_device.restype = i32
        L.zs_png_pack_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(i32), P(i32), P(vp), P(i32), P(vp), P(i32), i32, P(vp), P(i64), vp]
        L.zs_png_survey_batch_device.restype = i32
        L.zs_png_survey_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), i32, P(PngSurvey), vp]
        L.zs_png_choose_format.restype = i32
        L.zs_png_choose_format.argtypes = [P(PngSurvey), P(i32), P(i32)]
        L.zs_png_encode_rgba_batch_device.restype = i32
        L.zs_png_encode_rgba_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), i32, P(i32), P(i32), P(vp), P(i64), i64, i64, P(vp), P(i64),
                                                      P(i64), P(i32), P(i32), P(i32), i32, i32, i32, vp]
    if hasattr(L, "zs_png_compose_batch_device"):  # (an older build selected with ZS_LIB for an A/B run lacks animated PNG)
        L.zs_png_anim_info.restype = i32
        L.zs_png_anim_info.argtypes = [vp, i64, P(PngAnim), P(PngFrame), i32]
        L.zs_png_compose_batch_device.restype = i32
        L.zs_png_compose_batch_device.argtypes = [vp, i32, P(P(vp)), P(P(PngFrame)), P(i32), P(i64), P(i64), i32, P(vp), vp]
        L.zs_png_decode_anim_batch.restype = i32
        L.zs_png_decode_anim_batch.argtypes = [vp, i32, P(vp), P(i64), i32, P(vp), P(i64), P(PngAnim), P(i32), vp]
    if hasattr(L, "zs_png_diff_batch_device"):  # (an older build selected with ZS_LIB for an A/B run lacks the animated encoder)
        L.zs_png_diff_batch_device.restype = i32
        L.zs_png_diff_batch_device.argtypes = [vp, i32, P(vp), P(i32), P(i64), P(i64), i32, P(P(PngFrame)), vp]
        L.zs_png_crop_batch_device.restype = i32
        L.zs_png_crop_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(i64), P(i64), P(i64), i32, P(vp), vp]
        L.zs_png_anim_bound.restype = i64
        L.zs_png_anim_bound.argtypes = [i64, i64, i32, i32, i32, i64, i64]
        L.zs_png_encode_anim_batch_device.restype = i32
        L.zs_png_encode_anim_batch_device.argtypes = [vp, i32, P(vp), P(i32), P(i64), P(i64), i32, P(P(i32)), P(P(i32)), P(i32), P(i32), P(i32), P(vp), P(i64),
                                                      i64, i64, P(vp), P(i64), P(i64), P(i32), P(P(PngFrame)), P(i32), P(i32), i32, i32, i32, vp]
    if hasattr(L, "zs_inflate_wrap_batch_device"):  # (an older build selected with ZS_LIB for an A/B run lacks the containers)
        L.zs_wrap_bound.restype = i64
        L.zs_wrap_bound.argtypes = [i64, i32]
        L.zs_deflate_wrap_batch_device.restype = i32
        L.zs_deflate_wrap_batch_device.argtypes = batch_args + [i32, vp]
        L.zs_inflate_wrap_batch_device.restype = i32
        L.zs_inflate_wrap_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(vp), P(i64), P(i64), P(i64), P(i32), i32, vp]
        L.zs_gzip_file_info.restype = i32
        L.zs_gzip_file_info.argtypes = [vp, i64, P(GzipInfo)]
        L.zs_gzip_decode_files_batch.restype = i32
        L.zs_gzip_decode_files_batch.argtypes = [vp, i32, P(vp), P(i64), P(vp), P(i64), P(i64), P(i32), P(i32), vp]
    if hasattr(L, "zs_tiff_file_info"):
        L.zs_tiff_file_info.restype = i32
        L.zs_tiff_file_info.argtypes = [vp, i64, i64, P(TiffInfo), P(TiffChunk), i64]
        L.zs_tiff_unpredict_batch_device.restype = i32
        L.zs_tiff_unpredict_batch_device.argtypes = [vp, i32, P(vp), P(vp), P(i64), P(i64), P(i64), P(i64), P(i32), P(i32), P(i32), P(i32), vp]
        L.zs_tiff_predict_batch_device.restype = i32
        L.zs_tiff_predict_batch_device.argtypes = [vp, i32, P(vp), P(vp), P(i64), P(i64), P(i64), P(i64), P(i32), P(i32), P(i32), vp]
        L.zs_tiff_decode_files_batch.restype = i32
        L.zs_tiff_decode_files_batch.argtypes = [vp, i32, P(vp), P(i64), P(i64), P(vp), P(i64), P(i64), P(P(i32)), P(i32), vp]
        L.zs_tiff_bound.restype = i64
        L.zs_tiff_bound.argtypes = [P(TiffPut)]
        L.zs_tiff_encode_batch_device.restype = i32
        L.zs_tiff_encode_batch_device.argtypes = [vp, i32, P(TiffPut), P(vp), P(i64), P(i64), P(i32), i32, i32, i32, vp]
    if hasattr(L, "zs_exr_file_info"):
        L.zs_exr_file_info.restype = i32
        L.zs_exr_file_info.argtypes = [vp, i64, P(ExrInfo), P(ExrChannel), i64, P(ExrChunk), i64]
        L.zs_exr_unpredict_batch_device.restype = i32
        L.zs_exr_unpredict_batch_device.argtypes = [vp, i32, P(vp), P(vp), P(i64), vp]
        L.zs_exr_predict_batch_device.restype = i32
        L.zs_exr_predict_batch_device.argtypes = [vp, i32, P(vp), P(vp), P(i64), vp]
        L.zs_exr_decode_files_batch.restype = i32
        L.zs_exr_decode_files_batch.argtypes = [vp, i32, P(vp), P(i64), P(vp), P(i64), P(i64), P(P(i32)), P(i32), vp]
        L.zs_exr_bound.restype = i64
        L.zs_exr_bound.argtypes = [P(ExrPut)]
        L.zs_exr_encode_batch_device.restype = i32
        L.zs_exr_encode_batch_device.argtypes = [vp, i32, P(ExrPut), P(vp), P(i64), P(i64), P(i32), i32, i32, i32, vp]
    if hasattr(L, "zs_chunks_decode_batch"):
        L.zs_chunk_grid_info.restype = i32
        L.zs_chunk_grid_info.argtypes = [P(ChunkGrid), P(i64), P(i64), P(i64)]
        L.zs_chunks_decode_batch.restype = i32
        L.zs_chunks_decode_batch.argtypes = [vp, i32, P(ChunkGrid), P(P(ChunkRef)), P(vp), P(i64), P(P(i32)), P(i32), vp]
        L.zs_chunks_bound.restype = i64
        L.zs_chunks_bound.argtypes = [P(ChunkGrid)]
        L.zs_chunks_encode_batch_device.restype = i32
        L.zs_chunks_encode_batch_device.argtypes = [vp, i32, P(ChunkGrid), P(vp), P(vp), P(i64), P(i64), P(P(i64)), P(P(i64)), P(P(i32)), P(i32), i32, i32,
                                                    i32, i32, vp]
        L.zs_shuffle_batch_device.restype = i32
        L.zs_shuffle_batch_device.argtypes = [vp, i32, P(vp), P(vp), P(i64), P(i32), vp]
        L.zs_unshuffle_batch_device.restype = i32
        L.zs_unshuffle_batch_device.argtypes = [vp, i32, P(vp), P(vp), P(i64), P(i32), vp]
    if hasattr(L, "zs_chunks_decode_filters_batch"):
        L.zs_chunks_decode_filters_batch.restype = i32
        L.zs_chunks_decode_filters_batch.argtypes = [vp, i32, P(ChunkGrid), P(ChunkFilters), P(P(ChunkRef)), P(vp), P(i64), P(P(i32)), P(i32), vp]
        L.zs_chunks_encode_filters_batch_device.restype = i32
        L.zs_chunks_encode_filters_batch_device.argtypes = [vp, i32, P(ChunkGrid), P(ChunkFilters), P(vp), P(vp), P(i64), P(i64), P(P(i64)), P(P(i64)), P(P(i32)),
                                                            P(i32), i32, i32, i32, i32, vp]
        L.zs_chunks_filters_bound.restype = i64
        L.zs_chunks_filters_bound.argtypes = [P(ChunkGrid), P(ChunkFilters)]
        L.zs_fletcher32_batch_device.restype = i32
        L.zs_fletcher32_batch_device.argtypes = [vp, i32, P(vp), P(i64), P(ctypes.c_uint32), vp]
        L.zs_delta_encode_batch_device.restype = i32
        L.zs_delta_encode_batch_device.argtypes = [vp, i32, P(vp), P(vp), P(i64), P(i32), vp]
        L.zs_delta_decode_batch_device.restype = i32
        L.zs_delta_decode_batch_device.argtypes = [vp, i32, P(vp), P(vp), P(i64), P(i32), vp]
    if hasattr(L, "zs_zip_file_info"):
        L.zs_zip_file_info.restype = i32
        L.zs_zip_file_info.argtypes = [vp, i64, P(ZipInfo), P(ZipEntry), i64]
        L.zs_zip_decode_files_batch.restype = i32
        L.zs_zip_decode_files_batch.argtypes = [vp, i32, P(vp), P(i64), P(vp), P(i64), P(i64), P(P(i32)), P(i32), vp]
        L.zs_zip_bound.restype = i64
        L.zs_zip_bound.argtypes = [P(ZipPut), i32]
        L.zs_zip_encode_batch_device.restype = i32
        L.zs_zip_encode_batch_device.argtypes = [vp, i32, P(P(ZipPut)), P(i32), P(vp), P(i64), P(i64), P(i32), i32, i32, i32, vp]
    _lib = L
    return L
