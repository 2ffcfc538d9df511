"""zlibstream_amd -- MI355X (gfx950) deflate engine behind the ZlibStream API.

Host-side mirror of the reference's public surface (ZlibOutputStream,
ZlibOptions, CompressionLevel, CompressionStrategy, FlushMode,
ZlibStreamException) over the C ABI in include/zsgpu.h.  The compression path
has no CPU fallback: it needs libzsgpu.so and an MI355X.
"""
from .api import (CompressionLevel, CompressionState, CompressionStrategy, Engine, FlushMode, ZlibInputStream, ZlibOptions,  # noqa: F401
                  ZlibOutputStream, ZlibStreamException, compress, deflate_batch_multi, deflate_batch_multi_device, deflate_bound,
                  device_count, inflate_batch_multi, inflate_batch_multi_device, png_filter_batch_device, png_filter_device, png_idat_batch_device,
                  png_unfilter_batch_device, png_unfilter_device, png_idat_layout, png_adam7_merge_batch_device, png_decode_batch_device,
                  crc32_device, crc32_batch_device, png_file_bound, png_encode_batch_device, png_file_info, png_decode_files_batch,
                  png_expand_batch_device, png_file_colors, png_decode_files_rgba_batch, PNG_RGBA8, PNG_RGBA16,
                  png_adam7_split_batch_device, png_idat_interlace_batch_device, png_encode_interlace_batch_device,
                  png_pack_batch_device, png_survey_batch_device, png_choose_format, png_encode_rgba_batch_device,
                  png_anim_info, png_compose_batch_device, png_decode_anim_batch, PNG_DISPOSE_NONE, PNG_DISPOSE_BACKGROUND,
                  PNG_DISPOSE_PREVIOUS, PNG_BLEND_SOURCE, PNG_BLEND_OVER, png_diff_batch_device, png_crop_batch_device,
                  png_anim_bound, png_encode_anim_batch_device, WRAP_ZLIB, WRAP_RAW, WRAP_GZIP, wrap_bound,
                  deflate_wrap_batch_device, inflate_wrap_batch_device, gzip_file_info, gzip_decode_files_batch,
                  ZIP_AUTO, ZIP_STORED, ZIP_DEFLATED, zip_file_info, zip_decode_files_batch, zip_bound, zip_encode_batch_device,
                  tiff_file_info, tiff_decode_files, tiff_encode, tiff_bound, tiff_predict, tiff_unpredict,
                  exr_file_info, exr_decode_files, exr_encode, exr_bound, exr_predict, exr_unpredict,
                  CHUNK_STORED, CHUNK_UNSHUFFLED, CHUNK_SKIP, CHUNK_ABSENT, chunk_grid_info, chunks_decode, chunks_encode, chunks_bound,
                  shuffle, unshuffle, zarr_v2_grid, FLETCHER32_TILE, DELTA_TILE, chunks_filters_bound, fletcher32, delta_encode,
                  delta_decode, zarr_v2_filters)
