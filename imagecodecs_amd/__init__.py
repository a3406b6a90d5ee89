"""imagecodecs_amd -- MI355X-native JPEG codec behind ImageCodecs' codecs.h API.

The product is the C-ABI library ``imagecodecs_amd/lib/libicx.so`` (include/icx.h): hand-
written gfx950 HIP kernels for the NanoJPEG-exact decode path and the tiny_jpeg-exact
encode path. This module is the host-side mirror of the reference interface for Python
callers (tests, bench): it binds the C ABI with ctypes and offers

  * ``Context``                   -- one device + stream (icx_create)
  * ``Context.nj_decode`` & co.   -- njInit/njDecode/njGet* semantics (jpeg_dec.h:117-171)
  * ``Context.decode``            -- Image::readJpg's one-shot decode (codecs.cpp:821-849)
  * ``Batch``                     -- device-resident batched decode (the throughput path)
  * ``Context.hdr_decode``        -- Image::readHdr's Radiance RGBE -> float decode (codecs.cpp:706-777)
  * ``HdrBatch``                  -- device-resident batched .hdr decode
  * ``Context.hdr_encode``        -- Image::writeHdr's float -> Radiance RGBE write (codecs.cpp:779-818), RLE rows included
  * ``Context.png_decode``        -- Image::readPng's PNG -> RGBA8 decode (codecs.cpp:903-1020)
  * ``PngBatch``                  -- device-resident batched PNG decode
  * ``Context.exr_decode``        -- Image::readExr's OpenEXR -> RGBA float (tinyexr LoadEXRFromMemory)
  * ``Context.exr_encode``        -- Image::writeExr's float pixels -> OpenEXR (tinyexr SaveEXR)
  * ``Context.tga_decode`` / ``tga_encode`` -- Image::readTga / writeTga (codecs.cpp:1304-1437), RLE included
  * ``TgaBatch``                  -- device-resident batched .tga decode
  * ``Context.bmp_decode`` / ``bmp_save_to_memory`` -- Image::readBmp / writeBmp (codecs.cpp:255-375), RLE4/RLE8 and bitfields read
  * ``BmpBatch``                  -- device-resident batched .bmp decode
  * ``Context.gif_decode``        -- Image::readGif (codecs.cpp:507-542): first frame, wave LZW decode
  * ``GifBatch``                  -- device-resident batched .gif decode
  * ``Context.gif_save_to_memory`` / ``gif_encode_device_batch`` -- Image::writeGif: exact palette or a 6x7x6
    cube, the code stream cut into segments of one wave each
  * ``Context.tiff_decode``       -- Image::readTiff (codecs.cpp:1439-1484): strips / tiles, one wave per chunk
  * ``Context.tiff_save_to_memory`` / ``tiff_encode_device_batch`` -- Image::writeTiff (codecs.cpp:1485-1513):
    uncompressed, PackBits, LZW or Deflate strips
  * ``TiffBatch``                 -- device-resident batched .tif decode
  * ``Context.pnm_decode`` / ``pnm_encode`` -- Image::readPbm / writePbm (codecs.cpp:1034-1167): P1-P6, Pf, PF
  * ``PnmBatch``                  -- device-resident batched Netpbm decode
  * ``Context.dds_decode`` / ``dds_save_to_memory`` -- Image::readDds / writeDds: BC1-BC5 decode, masked and copied
                                     forms; uncompressed and range-fit BC (DXT1 / DXT5 / BC4U / BC5U) write
  * ``DdsBatch``                  -- device-resident batched .dds decode
  * ``Image``                     -- ImageCodecs::Image (codecs.h:16-103) for .jpg/.jpeg/.png/.hdr/.exr/.tga/.bmp/.gif/.tif
                                     and .pbm/.pgm/.ppm/.pnm/.pfm, .dds

There is deliberately no CPU fallback: if libicx.so is missing or no GPU is visible every
entry point raises ``ICXError``.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np

__all__ = ["ICXError", "Context", "Batch", "HdrBatch", "Image", "lib", "build", "LIB_PATH",
           "OK", "NO_JPEG", "UNSUPPORTED", "OUT_OF_MEM", "INTERNAL_ERR", "SYNTAX_ERROR",
           "HDR_OK", "HDR_NOT_RADIANCE", "HDR_BAD_HEADER", "HDR_MALFORMED", "HDR_TRUNCATED",
           "HDR_TOO_LARGE", "HDR_INVALID_ARGUMENT", "HDR_INTERNAL_ERR", "hdr_probe", "hdr_encode_bound", "exr_probe",
           "PngBatch", "png_probe", "PNGR_OK", "PNGR_NOT_PNG", "PNGR_BAD_HEADER", "PNGR_UNSUPPORTED", "PNGR_MALFORMED",
           "PNGR_BAD_DATA", "PNGR_TOO_LARGE", "PNGR_INTERNAL_ERR", "EXR_SUCCESS", "EXR_INVALID_DATA", "Multi", "RECORD_DTYPE", "records_device",
           "checksum64", "multi_shard", "TgaBatch", "tga_probe", "tga_encode_bound", "TGA_OK", "TGA_BAD_HEADER",
           "TGA_UNSUPPORTED", "TGA_NO_IMAGE", "TGA_MALFORMED", "TGA_TRUNCATED", "TGA_TOO_LARGE", "TGA_INVALID_ARGUMENT",
           "TGA_INTERNAL_ERR", "BmpBatch", "bmp_probe", "bmp_encode_bound", "BMP_OK", "BMP_NOT_BMP", "BMP_BAD_HEADER",
           "BMP_UNSUPPORTED", "BMP_TRUNCATED", "BMP_TOO_LARGE", "BMP_INVALID_ARGUMENT", "BMP_INTERNAL_ERR", "GifBatch", "gif_probe", "GIF_OK", "GIF_NOT_GIF", "GIF_BAD_HEADER", "GIF_MALFORMED",
           "GIF_BAD_DATA", "GIF_TRUNCATED", "GIF_TOO_LARGE", "GIF_INVALID_ARGUMENT", "GIF_INTERNAL_ERR", "GIF_PALETTE_AUTO", "GIF_PALETTE_CUBE", "gif_encode_bound", "TiffBatch", "tiff_probe", "TIFF_OK",
           "TIFF_NOT_TIFF", "TIFF_BAD_HEADER", "TIFF_UNSUPPORTED", "TIFF_MALFORMED", "TIFF_BAD_DATA", "TIFF_TRUNCATED",
           "TIFF_TOO_LARGE", "TIFF_INVALID_ARGUMENT", "TIFF_INTERNAL_ERR", "TIFF_COMPRESSION_NONE", "TIFF_COMPRESSION_LZW",
           "TIFF_COMPRESSION_DEFLATE", "TIFF_COMPRESSION_PACKBITS", "tiff_encode_bound", "PnmBatch", "pnm_probe", "pnm_encode_bound", "PNM_OK", "PNM_NOT_PNM",
           "PNM_BAD_HEADER", "PNM_UNSUPPORTED", "PNM_BAD_DATA", "PNM_TRUNCATED", "PNM_TOO_LARGE", "PNM_INVALID_ARGUMENT",
           "PNM_INTERNAL_ERR", "PNM_UBYTE", "PNM_USHORT", "PNM_FLOAT", "PNM_P4", "PNM_P5", "PNM_P6", "PNM_PF",
           "PNM_ASCII_TILE", "DdsBatch", "dds_probe", "dds_encode_bound", "DDS_OK", "DDS_NOT_DDS", "DDS_BAD_HEADER",
           "DDS_UNSUPPORTED", "DDS_TRUNCATED", "DDS_TOO_LARGE", "DDS_INVALID_ARGUMENT", "DDS_INTERNAL_ERR", "DDS_RAW", "DDS_BC"]

OK, NO_JPEG, UNSUPPORTED, OUT_OF_MEM, INTERNAL_ERR, SYNTAX_ERROR = range(6)  # nj_result_t
RESULT_NAMES = ["NJ_OK", "NJ_NO_JPEG", "NJ_UNSUPPORTED", "NJ_OUT_OF_MEM", "NJ_INTERNAL_ERR", "NJ_SYNTAX_ERROR"]

_HERE = os.path.dirname(os.path.abspath(__file__))
# ICX_LIB selects another build of the same library (e.g. an instrumented variant); it is
# still the HIP library, there is no other implementation to select.
_DEFAULT_LIB = os.path.join(_HERE, "lib", "libicx.so")
LIB_PATH = os.environ.get("ICX_LIB") or _DEFAULT_LIB
_LIB = None


class ICXError(RuntimeError):
    pass


def build() -> str:
    """Compile libicx.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", "-C", _HERE], check=True)
    return LIB_PATH


_vp, _i32, _i64, _u64, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_size_t
_SIGS = {
    "icx_version": (C.c_char_p, []),
    "icx_last_error": (C.c_char_p, [_vp]),
    "icx_create": (_vp, [_i32]),
    "icx_destroy": (None, [_vp]),
    "icx_free": (None, [_vp]),
    "icx_jpeg_probe": (_i32, [_vp, _sz, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_nj_init": (None, [_vp]),
    "icx_nj_done": (None, [_vp]),
    "icx_nj_decode": (_i32, [_vp, _vp, _i32]),
    "icx_nj_get_width": (_i32, [_vp]),
    "icx_nj_get_height": (_i32, [_vp]),
    "icx_nj_is_color": (_i32, [_vp]),
    "icx_nj_get_image": (_vp, [_vp]),
    "icx_nj_get_image_size": (_i32, [_vp]),
    "icx_jpeg_decode": (_i32, [_vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_batch_create": (_vp, [_vp, _i32, _i32, _i32, _i32]),
    "icx_batch_destroy": (None, [_vp]),
    "icx_jpeg_batch_decode": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "icx_jpeg_batch_decode_host": (_i32, [_vp, _i32, _vp, _vp, _vp, _u64, _vp, _vp]),
    "icx_batch_stage_times": (_i32, [_vp, _vp, _vp, _i32]),
    "icx_batch_group": (_i32, [_vp]),
    "icx_batch_groups": (_i32, [_vp, _i32]),
    "icx_batch_path_stats": (_i32, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_batch_dri_stats": (_i32, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_tje_encode_with_func": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "icx_tje_encode_to_file_at_quality": (_i32, [_vp, C.c_char_p, _i32, _i32, _i32, _i32, _vp]),
    "icx_tje_encode_to_file": (_i32, [_vp, C.c_char_p, _i32, _i32, _i32, _vp]),
    "icx_jpeg_encode_with_func": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "icx_encoder_create": (_vp, [_vp]),
    "icx_encoder_destroy": (None, [_vp]),
    "icx_encoder_stage_times": (_i32, [_vp, _vp, _vp, _i32]),
    "icx_png_encode_with_func": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32]),
    "icx_png_save_to_file": (_i32, [_vp, C.c_char_p, _vp, _i32, _i32, _i32]),
    "icx_png_encoder_create": (_vp, [_vp]),
    "icx_png_encoder_destroy": (None, [_vp]),
    "icx_png_encode_device": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _u64, C.POINTER(_u64), _vp]),
    "icx_png_encode_device_batch": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _u64, _vp, _vp, _vp]),
    "icx_png_encoder_stage_times": (_i32, [_vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i32]),
    "icx_jpeg_encode_device": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _u64, C.POINTER(_u64), _vp]),
    "icx_jpeg_encode_device_batch": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _u64, _vp, _vp, _vp]),
    "icx_hdr_probe": (_i32, [_vp, _sz, C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_hdr_decode": (_i32, [_vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_hdr_batch_create": (_vp, [_vp, _i32, _i32, _i32]),
    "icx_hdr_batch_destroy": (None, [_vp]),
    "icx_hdr_batch_decode": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "icx_hdr_batch_stage_times": (_i32, [_vp, _vp, _vp, _i32]),
    "icx_hdr_batch_locate_stats": (_i32, [_vp, _vp, _vp, _i32]),
    "icx_hdr_encode_bound": (_sz, [_i32, _i32, _i32, _i32]),
    "icx_hdr_save_to_memory": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, C.POINTER(_vp), C.POINTER(_sz)]),
    "icx_hdr_save_to_file": (_i32, [_vp, C.c_char_p, _vp, _i32, _i32, _i32, _i32]),
    "icx_hdr_encode_device_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _u64, _vp, _vp, _vp]),
    "icx_png_probe": (_i32, [_vp, _sz, C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_png_decode": (_i32, [_vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_png_batch_create": (_vp, [_vp, _i32, _i32, _i32]),
    "icx_png_batch_destroy": (None, [_vp]),
    "icx_png_batch_decode": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "icx_png_batch_stage_times": (_i32, [_vp, _vp, _vp, _i32]),
    "icx_jpeg_records": (_i32, [_vp, _i32, _vp, _u64, _vp, _vp, _i32, _i32, _vp, _vp]),
    "icx_checksum64": (_u64, [_vp, _sz]),
    "icx_ctx_device": (_i32, [_vp]),
    "icx_ctx_stream": (_vp, [_vp]),
    "icx_multi_create": (_vp, [_vp, _i32, _i32, _i32]),
    "icx_multi_destroy": (None, [_vp]),
    "icx_multi_decode_host": (_i32, [_vp, _i32, _vp, _vp, _vp, _u64, _vp, _vp]),
    "icx_multi_last_error": (C.c_char_p, [_vp]),
    "icx_multi_gather": (C.c_char_p, [_vp]),
    "icx_multi_shard": (_i32, [_vp, _i32, _i32, _vp]),
    "icx_exr_probe": (_i32, [_vp, _sz, C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_exr_decode": (_i32, [_vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_exr_decode_device": (_i32, [_vp, _vp, _vp, _sz, _vp, _sz, C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_exr_decode_device_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "icx_exr_save_to_memory": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, C.POINTER(_vp), C.POINTER(_sz)]),
    "icx_exr_save_to_file": (_i32, [_vp, C.c_char_p, _vp, _i32, _i32, _i32, _i32]),
    "icx_exr_encode_bound": (_sz, [_i32, _i32, _i32, _i32]),
    "icx_exr_encode_device": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, C.POINTER(_sz)]),
    "icx_exr_encode_device_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "icx_tga_probe": (_i32, [_vp, _sz, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_tga_decode": (_i32, [_vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_tga_batch_create": (_vp, [_vp, _i32, _i32, _i32]),
    "icx_tga_batch_destroy": (None, [_vp]),
    "icx_tga_batch_decode": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "icx_tga_batch_stage_times": (_i32, [_vp, _vp, _vp, _i32]),
    "icx_gif_probe": (_i32, [_vp, _sz, C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_gif_decode": (_i32, [_vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_gif_batch_create": (_vp, [_vp, _i32, _i32, _i32]),
    "icx_gif_batch_destroy": (None, [_vp]),
    "icx_gif_batch_decode": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "icx_gif_batch_stage_times": (_i32, [_vp, _vp, _vp, _i32]),
    "icx_tiff_probe": (_i32, [_vp, _sz, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_tiff_decode": (_i32, [_vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_tiff_batch_create": (_vp, [_vp, _i32, _i32, _i32]),
    "icx_tiff_batch_destroy": (None, [_vp]),
    "icx_tiff_batch_decode": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "icx_tiff_batch_stage_times": (_i32, [_vp, _vp, _vp, _i32]),
    "icx_gif_encode_bound": (_sz, [_i32, _i32, _i32]),
    "icx_gif_save_to_memory": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_vp), C.POINTER(_sz)]),
    "icx_gif_save_to_file": (_i32, [_vp, C.c_char_p, _vp, _i32, _i32, _i32, _i32, _i32, _i32]),
    "icx_gif_encode_device_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _u64, _vp, _vp, _vp]),
    "icx_tiff_encode_bound": (_sz, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "icx_tiff_save_to_memory": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_vp), C.POINTER(_sz)]),
    "icx_tiff_save_to_file": (_i32, [_vp, C.c_char_p, _vp, _i32, _i32, _i32, _i32, _i32, _i32]),
    "icx_tiff_encode_device_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _u64, _vp, _vp, _vp]),
    "icx_tga_encode_bound": (_sz, [_i32, _i32, _i32]),
    "icx_tga_save_to_memory": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, C.POINTER(_vp), C.POINTER(_sz)]),
    "icx_tga_save_to_file": (_i32, [_vp, C.c_char_p, _vp, _i32, _i32, _i32, _i32]),
    "icx_tga_encode_device_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _u64, _vp, _vp, _vp]),
    "icx_bmp_probe": (_i32, [_vp, _sz, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_bmp_decode": (_i32, [_vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "icx_bmp_batch_create": (_vp, [_vp, _i32, _i32, _i32]),
    "icx_bmp_batch_destroy": (None, [_vp]),
    "icx_bmp_batch_decode": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "icx_bmp_batch_stage_times": (_i32, [_vp, _vp, _vp, _i32]),
    "icx_bmp_encode_bound": (_sz, [_i32, _i32, _i32]),
    "icx_bmp_save_to_memory": (_i32, [_vp, _vp, _i32, _i32, _i32, C.POINTER(_vp), C.POINTER(_sz)]),
    "icx_bmp_save_to_file": (_i32, [_vp, C.c_char_p, _vp, _i32, _i32, _i32]),
    "icx_bmp_encode_device_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _u64, _vp, _vp, _vp]),
    "icx_dds_probe": (_i32, [_vp, _sz] + [C.POINTER(_i32)] * 4),
    "icx_dds_decode": (_i32, [_vp, _vp, _sz, C.POINTER(_vp)] + [C.POINTER(_i32)] * 4),
    "icx_dds_batch_create": (_vp, [_vp, _i32, _i32, _i32]),
    "icx_dds_batch_destroy": (None, [_vp]),
    "icx_dds_batch_decode": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "icx_dds_batch_stage_times": (_i32, [_vp, _vp, _vp, _i32]),
    "icx_dds_encode_bound": (_sz, [_i32, _i32, _i32, _i32]),
    "icx_dds_save_to_memory": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, C.POINTER(_vp), C.POINTER(_sz)]),
    "icx_dds_save_to_file": (_i32, [_vp, C.c_char_p, _vp, _i32, _i32, _i32, _i32]),
    "icx_dds_encode_device_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _u64, _vp, _vp, _vp]),
    "icx_pnm_probe": (_i32, [_vp, _sz] + [C.POINTER(_i32)] * 5),
    "icx_pnm_decode": (_i32, [_vp, _vp, _sz, C.POINTER(_vp)] + [C.POINTER(_i32)] * 5),
    "icx_pnm_batch_create": (_vp, [_vp, _i32, _i32, _i32]),
    "icx_pnm_batch_destroy": (None, [_vp]),
    "icx_pnm_batch_decode": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "icx_pnm_batch_stage_times": (_i32, [_vp, _vp, _vp, _i32]),
    "icx_pnm_encode_bound": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "icx_pnm_save_to_memory": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(_vp), C.POINTER(_sz)]),
    "icx_pnm_save_to_file": (_i32, [_vp, C.c_char_p, _vp, _i32, _i32, _i32, _i32, _i32]),
    "icx_pnm_encode_device_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _u64, _vp, _vp, _vp]),
}

# icx_record (include/icx.h): per-image result record gathered across devices / ranks
RECORD_DTYPE = np.dtype([("status", "<i4"), ("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"),
                         ("checksum", "<u8")])

# icx_hdr_result (include/icx.h): Image::readHdr outcomes
HDR_OK, HDR_NOT_RADIANCE, HDR_BAD_HEADER, HDR_MALFORMED, HDR_TRUNCATED, HDR_TOO_LARGE = range(6)
HDR_INVALID_ARGUMENT = 6  # the write's refused arguments
HDR_INTERNAL_ERR = -1

# icx_png_read_result (include/icx.h): Image::readPng outcomes
PNGR_OK, PNGR_NOT_PNG, PNGR_BAD_HEADER, PNGR_UNSUPPORTED, PNGR_MALFORMED, PNGR_BAD_DATA, PNGR_TOO_LARGE = range(7)
PNGR_INTERNAL_ERR = -1

# icx_exr_result (include/icx.h): tinyexr's LoadEXRFromMemory codes
EXR_SUCCESS, EXR_INVALID_MAGIC_NUMBER, EXR_INVALID_EXR_VERSION, EXR_INVALID_ARGUMENT, EXR_INVALID_DATA = 0, -1, -2, -3, -4
EXR_UNSUPPORTED_FORMAT, EXR_INVALID_HEADER, EXR_UNSUPPORTED_FEATURE, EXR_INTERNAL_ERR = -8, -9, -10, -100

# icx_tga_result (include/icx.h): Image::readTga / writeTga outcomes
(TGA_OK, TGA_BAD_HEADER, TGA_UNSUPPORTED, TGA_NO_IMAGE, TGA_MALFORMED, TGA_TRUNCATED, TGA_TOO_LARGE,
 TGA_INVALID_ARGUMENT) = range(8)
TGA_INTERNAL_ERR = -1
# icx_bmp_result (include/icx.h): Image::readBmp / writeBmp outcomes
(BMP_OK, BMP_NOT_BMP, BMP_BAD_HEADER, BMP_UNSUPPORTED, BMP_TRUNCATED, BMP_TOO_LARGE, BMP_INVALID_ARGUMENT) = range(7)
BMP_INTERNAL_ERR = -1
# icx_gif_result (include/icx.h): Image::readGif outcomes
GIF_OK, GIF_NOT_GIF, GIF_BAD_HEADER, GIF_MALFORMED, GIF_BAD_DATA, GIF_TRUNCATED, GIF_TOO_LARGE = range(7)
GIF_INVALID_ARGUMENT = 7  # the write only
GIF_INTERNAL_ERR = -1
GIF_PALETTE_AUTO, GIF_PALETTE_CUBE = 0, 1
# icx_tiff_result (include/icx.h): Image::readTiff / writeTiff outcomes
(TIFF_OK, TIFF_NOT_TIFF, TIFF_BAD_HEADER, TIFF_UNSUPPORTED, TIFF_MALFORMED, TIFF_BAD_DATA, TIFF_TRUNCATED,
 TIFF_TOO_LARGE, TIFF_INVALID_ARGUMENT) = range(9)
TIFF_INTERNAL_ERR = -1
# icx_tiff_compression: what writeTiff can write
TIFF_COMPRESSION_NONE, TIFF_COMPRESSION_LZW, TIFF_COMPRESSION_DEFLATE, TIFF_COMPRESSION_PACKBITS = 1, 5, 8, 32773
# icx_pnm_result (include/icx.h): Image::readPbm / writePbm outcomes
(PNM_OK, PNM_NOT_PNM, PNM_BAD_HEADER, PNM_UNSUPPORTED, PNM_BAD_DATA, PNM_TRUNCATED, PNM_TOO_LARGE,
 PNM_INVALID_ARGUMENT) = range(8)
PNM_INTERNAL_ERR = -1
PNM_UBYTE, PNM_USHORT, PNM_FLOAT = range(3)  # icx_pnm_type = ImageCodecs::Type
PNM_P4, PNM_P5, PNM_P6, PNM_PF = 4, 5, 6, 8  # icx_pnm_format
PNM_ASCII_TILE = 4096  # icx_pnm_core.h kPnmTile: bytes of raster text per tile of the P1 / P2 / P3 read
_PNM_DTYPES = (np.uint8, np.uint16, np.float32)
# icx_dds_result (include/icx.h): Image::readDds / writeDds outcomes
(DDS_OK, DDS_NOT_DDS, DDS_BAD_HEADER, DDS_UNSUPPORTED, DDS_TRUNCATED, DDS_TOO_LARGE, DDS_INVALID_ARGUMENT) = range(7)
DDS_INTERNAL_ERR = -1
DDS_RAW, DDS_BC = 0, 1  # icx_dds_format

WRITE_FUNC = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int)


def _share_hip_runtime_with_torch() -> None:
    """PyTorch-ROCm ships its own libamdhip64/libhsa-runtime64 and loads them by file name
    (RPATH $ORIGIN). Preloading exactly those files first makes libicx's DT_NEEDED
    (libamdhip64.so.7 / libhsa-runtime64.so.1, matched by SONAME) bind to the same runtime,
    so device pointers, streams and RCCL are shared whatever the import order."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    tlib = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(tlib, name)
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)


def lib():
    """Load libicx.so (raises ICXError if it has not been built)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ICXError(f"{LIB_PATH} not built: run `make -C imagecodecs_amd` (hipcc, gfx950)")
        _share_hip_runtime_with_torch()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                if LIB_PATH != _DEFAULT_LIB:
                    continue  # (an older build loaded by ICX_LIB for an A/B: that entry is unusable)
                raise
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def _err(ctx_ptr) -> str:
    msg = lib().icx_last_error(ctx_ptr)
    return msg.decode() if msg else ""


class Context:
    """icx_create(device): a device + HIP stream; also holds njDecode-style state."""

    def __init__(self, device: int = 0):
        self._p = lib().icx_create(device)
        if not self._p:
            raise ICXError("icx_create failed: " + _err(None))
        self.device = device

    def close(self):
        if getattr(self, "_p", None):
            lib().icx_destroy(self._p)
            self._p = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def ptr(self):
        return self._p

    # ---- NanoJPEG-compatible state API (jpeg_dec.h:130-171)
    def nj_init(self):
        lib().icx_nj_init(self._p)

    def nj_done(self):
        lib().icx_nj_done(self._p)

    def nj_decode(self, jpeg: bytes) -> int:
        buf = C.create_string_buffer(bytes(jpeg), max(1, len(jpeg)))
        return lib().icx_nj_decode(self._p, buf, len(jpeg))

    def nj_get_width(self) -> int:
        return lib().icx_nj_get_width(self._p)

    def nj_get_height(self) -> int:
        return lib().icx_nj_get_height(self._p)

    def nj_is_color(self) -> int:
        return lib().icx_nj_is_color(self._p)

    def nj_get_image_size(self) -> int:
        return lib().icx_nj_get_image_size(self._p)

    def nj_get_image(self) -> bytes:
        p = lib().icx_nj_get_image(self._p)
        return C.string_at(p, self.nj_get_image_size()) if p else b""

    # ---- one-shot decode (Image::readJpg)
    def decode(self, jpeg: bytes):
        """-> (code, width, height, ncomp, pixel bytes)."""
        buf = C.create_string_buffer(bytes(jpeg), max(1, len(jpeg)))
        out = C.c_void_p()
        w, h, n = C.c_int(), C.c_int(), C.c_int()
        code = lib().icx_jpeg_decode(self._p, buf, len(jpeg), C.byref(out), C.byref(w), C.byref(h), C.byref(n))
        pix = b""
        if out.value:
            pix = C.string_at(out.value, w.value * h.value * n.value)
            lib().icx_free(out)
        if code == INTERNAL_ERR and _err(self._p):
            raise ICXError(_err(self._p))
        return code, w.value, h.value, n.value, pix

    # ---- encode (tiny_jpeg, jpeg_enc.h:114-160)
    def tje_encode(self, quality: int, width: int, height: int, comps: int, src: bytes):
        """tje_encode_with_func into memory -> bytes, or None on error (tje returns 0)."""
        chunks = []

        @WRITE_FUNC
        def sink(_ctx, data, size):
            chunks.append(C.string_at(data, size))

        buf = C.create_string_buffer(bytes(src), max(1, len(src)))
        ok = lib().icx_tje_encode_with_func(self._p, sink, None, quality, width, height, comps, buf)
        return b"".join(chunks) if ok == 1 else None

    def _decode_image(self, entry: str, internal: int, data: bytes, k: int, depth=None, dtype=np.uint8):
        """The one-shot reads' ctypes side: entry(ctx, data, size, &out, k ints) -> (code, the k ints,
        array (h, w, d) of dtype or None). The ints start with w, h; d is `depth`, or the third int."""
        buf = C.create_string_buffer(bytes(data), max(1, len(data)))
        out = C.c_void_p()
        v = [C.c_int() for _ in range(k)]
        code = getattr(lib(), entry)(self._p, buf, len(data), C.byref(out), *[C.byref(x) for x in v])
        if code == internal:
            raise ICXError(entry + ": " + _err(self._p))
        v = [x.value for x in v]
        arr = None
        if out.value:
            w, h, d = v[0], v[1], depth or v[2]
            nbytes = w * h * d * np.dtype(dtype).itemsize
            arr = np.frombuffer(C.string_at(out.value, nbytes), dtype).reshape(h, w, d).copy()
            lib().icx_free(out)
        return (code, *v, arr)

    def hdr_decode(self, data: bytes):
        """Image::readHdr (codecs.cpp:706-777) on the GPU -> (code, w, h, rows, float32 (h, w, 4) or
        None). Rows past `rows` (a truncated file) are zero; code is an icx_hdr_result."""
        return self._decode_image("icx_hdr_decode", HDR_INTERNAL_ERR, data, 3, 4, np.float32)

    def hdr_encode(self, arr, rle: bool = False):
        """Image::writeHdr (codecs.cpp:779-818; contract in include/icx.h) on the GPU: float32 (h, w, 4)
        R, G, B, E as the read returns them, or (h, w, 3) plain R, G, B -> (code, the file's bytes or
        None). rle: rows run-length coded where the width allows (8..32767)."""
        a = np.ascontiguousarray(arr, np.float32)
        if a.ndim != 3:
            return HDR_INVALID_ARGUMENT, None
        h, w, d = a.shape
        out, size = C.c_void_p(), C.c_size_t()
        code = lib().icx_hdr_save_to_memory(self._p, a.ctypes.data if a.size else None, w, h, d, 1 if rle else 0,
                                            C.byref(out), C.byref(size))
        if code == HDR_INTERNAL_ERR:
            raise ICXError("icx_hdr_save_to_memory: " + _err(self._p))
        if code != HDR_OK:
            return code, None
        data = C.string_at(out.value, size.value)
        lib().icx_free(out)
        return code, data

    def hdr_encode_device_batch(self, d_srcs, widths, heights, d: int, rle: bool, d_out: int, out_stride: int,
                                d_sizes: int, d_status: int, stream=0) -> int:
        """icx_hdr_encode_device_batch: image i's floats at device address d_srcs[i], its file to
        d_out + i*out_stride, size (uint64) and status (int32) to the device arrays -> the call's code."""
        n = len(d_srcs)
        sp = (C.c_void_p * max(1, n))(*d_srcs)
        ws = np.ascontiguousarray(widths, np.int32)
        hs = np.ascontiguousarray(heights, np.int32)
        rc = lib().icx_hdr_encode_device_batch(self._p, n, sp, ws.ctypes.data, hs.ctypes.data, d, 1 if rle else 0, d_out,
                                               out_stride, d_sizes, d_status, stream or None)
        if rc == HDR_INTERNAL_ERR:
            raise ICXError("icx_hdr_encode_device_batch: " + _err(self._p))
        return rc

    def png_decode(self, data: bytes):
        """Image::readPng (codecs.cpp:903-1020) on the GPU -> (code, w, h, uint8 (h, w, 4) RGBA or
        None); code is an icx_png_read_result."""
        return self._decode_image("icx_png_decode", PNGR_INTERNAL_ERR, data, 2, 4)

    def exr_decode(self, data: bytes):
        """Image::readExr's LoadEXRFromMemory (tinyexr.h:6645) on the GPU -> (code, w, h, float32
        (h, w, 4) RGBA or None); code is an icx_exr_result (tinyexr's codes)."""
        buf = C.create_string_buffer(bytes(data), max(1, len(data)))
        out = C.c_void_p()
        w, h = C.c_int(), C.c_int()
        code = lib().icx_exr_decode(self._p, buf, len(data), C.byref(out), C.byref(w), C.byref(h))
        if code == EXR_INTERNAL_ERR:
            raise ICXError("icx_exr_decode: " + _err(self._p))
        arr = None
        if out.value:
            n = w.value * h.value * 4
            arr = np.frombuffer(C.string_at(out.value, n * 4), np.float32).reshape(h.value, w.value, 4).copy()
            lib().icx_free(out)
        return code, w.value, h.value, arr

    def exr_decode_device(self, data: bytes, d_data: int, d_out: int, out_floats: int):
        """icx_exr_decode_device: the file resident on the device at ``d_data`` (its ``len(data)``
        bytes + 16 zero bytes; ``data`` is the host copy the header is planned from), RGBA floats to
        device memory ``d_out`` -> (code, w, h)."""
        buf = C.create_string_buffer(bytes(data), max(1, len(data)))
        w, h = C.c_int(), C.c_int()
        code = lib().icx_exr_decode_device(self._p, buf, C.c_void_p(d_data), len(data), C.c_void_p(d_out), out_floats,
                                           C.byref(w), C.byref(h))
        if code == EXR_INTERNAL_ERR:
            raise ICXError("icx_exr_decode_device: " + _err(self._p))
        return code, w.value, h.value

    def exr_decode_device_batch(self, datas, d_ptrs, d_outs, out_floats):
        """icx_exr_decode_device_batch over n files (host copies ``datas``, device copies at
        ``d_ptrs`` each followed by 16 zero bytes, outputs at ``d_outs`` with ``out_floats`` room
        each) -> (codes, widths, heights) as int32 arrays."""
        n = len(datas)
        bufs = [C.create_string_buffer(bytes(d), max(1, len(d))) for d in datas]
        hp = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs])
        dp = (C.c_void_p * n)(*d_ptrs)
        sz = (C.c_size_t * n)(*[len(d) for d in datas])
        op = (C.c_void_p * n)(*d_outs)
        of = (C.c_size_t * n)(*out_floats)
        codes = np.zeros(n, np.int32)
        ws = np.zeros(n, np.int32)
        hs = np.zeros(n, np.int32)
        rc = lib().icx_exr_decode_device_batch(self._p, n, hp, dp, sz, op, of, codes.ctypes.data, ws.ctypes.data,
                                               hs.ctypes.data)
        if rc == EXR_INTERNAL_ERR:
            raise ICXError("icx_exr_decode_device_batch: " + _err(self._p))
        if rc != 0:
            raise ICXError(f"icx_exr_decode_device_batch: code {rc}")
        return codes, ws, hs

    def exr_encode(self, arr, fp16: bool = False) -> bytes:
        """Image::writeExr's SaveEXR (tinyexr.h:9333) on the GPU: float32 (h, w) or (h, w, c) with
        c in 1, 3, 4 -> the file's bytes. Raises ICXError with the icx_exr_result otherwise."""
        a = np.ascontiguousarray(arr, np.float32)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            raise ICXError(f"icx_exr_save_to_memory: code {EXR_INVALID_ARGUMENT}")
        h, w, c = a.shape
        out, size = C.c_void_p(), C.c_size_t()
        code = lib().icx_exr_save_to_memory(self._p, a.ctypes.data, w, h, c, 1 if fp16 else 0, C.byref(out),
                                            C.byref(size))
        if code == EXR_INTERNAL_ERR:
            raise ICXError("icx_exr_save_to_memory: " + _err(self._p))
        if code != EXR_SUCCESS:
            raise ICXError(f"icx_exr_save_to_memory: code {code}")
        data = C.string_at(out.value, size.value)
        lib().icx_free(out)
        return data

    def exr_encode_device(self, d_src: int, width: int, height: int, components: int, fp16: bool, d_out: int,
                          cap: int):
        """icx_exr_encode_device: ``width*height*components`` floats on the device at ``d_src``, the
        file to device memory ``d_out`` (``cap`` bytes of room) -> (code, size)."""
        size = C.c_size_t()
        code = lib().icx_exr_encode_device(self._p, C.c_void_p(d_src), width, height, components, 1 if fp16 else 0,
                                           C.c_void_p(d_out), cap, C.byref(size))
        return code, size.value

    def exr_encode_device_batch(self, d_srcs, widths, heights, components: int, fp16: bool, d_outs, caps):
        """icx_exr_encode_device_batch over n images -> (codes int32, sizes uint64)."""
        n = len(d_srcs)
        sp = (C.c_void_p * n)(*d_srcs)
        op = (C.c_void_p * n)(*d_outs)
        cp = (C.c_size_t * n)(*caps)
        ws = np.asarray(widths, np.int32)
        hs = np.asarray(heights, np.int32)
        codes = np.zeros(n, np.int32)
        sizes = (C.c_size_t * n)()
        rc = lib().icx_exr_encode_device_batch(self._p, n, sp, ws.ctypes.data, hs.ctypes.data, components,
                                               1 if fp16 else 0, op, cp, codes.ctypes.data, sizes)
        if rc == EXR_INTERNAL_ERR:
            raise ICXError("icx_exr_encode_device_batch: " + _err(self._p))
        if rc != 0:
            raise ICXError(f"icx_exr_encode_device_batch: code {rc}")
        return codes, np.array(list(sizes), np.uint64)

    def tga_decode(self, data: bytes):
        """Image::readTga (codecs.cpp:1304-1407; contract in include/icx.h) on the GPU -> (code, w, h,
        channels, uint8 (h, w, channels) or None); code is an icx_tga_result."""
        return self._decode_image("icx_tga_decode", TGA_INTERNAL_ERR, data, 3)

    def gif_decode(self, data: bytes):
        """Image::readGif (codecs.cpp:507-542; contract in include/icx.h) on the GPU -> (code, w, h,
        uint8 (h, w, 3) or None); code is an icx_gif_result."""
        return self._decode_image("icx_gif_decode", GIF_INTERNAL_ERR, data, 2, 3)

    def tiff_decode(self, data: bytes):
        """Image::readTiff (codecs.cpp:1439-1484; contract in include/icx.h) on the GPU -> (code, w, h,
        d, uint8 (h, w, d) or None); code is an icx_tiff_result."""
        return self._decode_image("icx_tiff_decode", TIFF_INTERNAL_ERR, data, 3)

    def tga_encode(self, px, rle: bool = False):
        """Image::writeTga (codecs.cpp:1410-1437) on the GPU: uint8 (h, w) or (h, w, d), d in 1, 3, 4,
        rows top-down -> (code, the file's bytes or None). rle: the run-length coded extension."""
        a = np.ascontiguousarray(px, np.uint8)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            return TGA_INVALID_ARGUMENT, None
        h, w, d = a.shape
        out, size = C.c_void_p(), C.c_size_t()
        code = lib().icx_tga_save_to_memory(self._p, a.ctypes.data if a.size else None, w, h, d, 1 if rle else 0,
                                            C.byref(out), C.byref(size))
        if code == TGA_INTERNAL_ERR:
            raise ICXError("icx_tga_save_to_memory: " + _err(self._p))
        if code != TGA_OK:
            return code, None
        data = C.string_at(out.value, size.value)
        lib().icx_free(out)
        return code, data

    def tga_encode_device_batch(self, d_srcs, widths, heights, d: int, rle: bool, d_out: int, out_stride: int,
                                d_sizes: int, d_status: int, stream=0) -> int:
        """icx_tga_encode_device_batch: image i's pixels at device address d_srcs[i], its file to
        d_out + i*out_stride, size (uint64) and status (int32) to the device arrays -> the call's code."""
        n = len(d_srcs)
        sp = (C.c_void_p * max(1, n))(*d_srcs)
        ws = np.ascontiguousarray(widths, np.int32)
        hs = np.ascontiguousarray(heights, np.int32)
        rc = lib().icx_tga_encode_device_batch(self._p, n, sp, ws.ctypes.data, hs.ctypes.data, d, 1 if rle else 0, d_out,
                                               out_stride, d_sizes, d_status, stream or None)
        if rc == TGA_INTERNAL_ERR:
            raise ICXError("icx_tga_encode_device_batch: " + _err(self._p))
        return rc

    def tiff_save_to_memory(self, px, compression: int = TIFF_COMPRESSION_DEFLATE, predictor: int = 1, rows_per_strip: int = 0):
        """Image::writeTiff on the GPU (contract in include/icx.h, "TIFF write"): uint8 (h, w) or
        (h, w, d), d in 1, 3, 4, rows top-down -> (code, the file's bytes or None)."""
        a = np.ascontiguousarray(px)
        if a.dtype != np.uint8:
            return TIFF_INVALID_ARGUMENT, None
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            return TIFF_INVALID_ARGUMENT, None
        h, w, d = a.shape
        out, size = C.c_void_p(), C.c_size_t()
        code = lib().icx_tiff_save_to_memory(self._p, a.ctypes.data if a.size else None, w, h, d, compression, predictor,
                                             rows_per_strip, C.byref(out), C.byref(size))
        if code == TIFF_INTERNAL_ERR:
            raise ICXError("icx_tiff_save_to_memory: " + _err(self._p))
        if code != TIFF_OK:
            return code, None
        data = C.string_at(out.value, size.value)
        lib().icx_free(out)
        return code, data

    def tiff_encode_device_batch(self, d_srcs, widths, heights, d: int, compression: int, predictor: int,
                                 rows_per_strip: int, d_out: int, out_stride: int, d_sizes: int, d_status: int,
                                 stream=0) -> int:
        """icx_tiff_encode_device_batch: image i's pixels at device address d_srcs[i], its file to
        d_out + i*out_stride, size (uint64) and status (int32) to the device arrays -> the call's code."""
        n = len(d_srcs)
        sp = (C.c_void_p * max(1, n))(*d_srcs)
        ws = np.ascontiguousarray(widths, np.int32)
        hs = np.ascontiguousarray(heights, np.int32)
        rc = lib().icx_tiff_encode_device_batch(self._p, n, sp, ws.ctypes.data, hs.ctypes.data, d, compression, predictor,
                                                rows_per_strip, d_out, out_stride, d_sizes, d_status, stream or None)
        if rc == TIFF_INTERNAL_ERR:
            raise ICXError("icx_tiff_encode_device_batch: " + _err(self._p))
        return rc

    def gif_save_to_memory(self, px, segment_pixels: int = 0, dither: bool = False, palette_mode: int = GIF_PALETTE_AUTO):
        """Image::writeGif on the GPU (contract in include/icx.h, "GIF write"): uint8 (h, w) or
        (h, w, d), d in 1, 3, 4, rows top-down -> (code, the file's bytes or None)."""
        a = np.ascontiguousarray(px)
        if a.dtype != np.uint8:
            return GIF_INVALID_ARGUMENT, None
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            return GIF_INVALID_ARGUMENT, None
        h, w, d = a.shape
        out, size = C.c_void_p(), C.c_size_t()
        code = lib().icx_gif_save_to_memory(self._p, a.ctypes.data if a.size else None, w, h, d, segment_pixels, int(dither),
                                            palette_mode, C.byref(out), C.byref(size))
        if code == GIF_INTERNAL_ERR:
            raise ICXError("icx_gif_save_to_memory: " + _err(self._p))
        if code != GIF_OK:
            return code, None
        data = C.string_at(out.value, size.value)
        lib().icx_free(out)
        return code, data

    def gif_encode_device_batch(self, d_srcs, widths, heights, d: int, segment_pixels: int, dither: int, palette_mode: int,
                                d_out: int, out_stride: int, d_sizes: int, d_status: int, stream=0) -> int:
        """icx_gif_encode_device_batch: image i's pixels at device address d_srcs[i], its file to
        d_out + i*out_stride, size (uint64) and status (int32) to the device arrays -> the call's code."""
        n = len(d_srcs)
        sp = (C.c_void_p * max(1, n))(*d_srcs)
        ws = np.ascontiguousarray(widths, np.int32)
        hs = np.ascontiguousarray(heights, np.int32)
        rc = lib().icx_gif_encode_device_batch(self._p, n, sp, ws.ctypes.data, hs.ctypes.data, d, segment_pixels, int(dither),
                                               palette_mode, d_out, out_stride, d_sizes, d_status, stream or None)
        if rc == GIF_INTERNAL_ERR:
            raise ICXError("icx_gif_encode_device_batch: " + _err(self._p))
        return rc

    def bmp_decode(self, data: bytes):
        """Image::readBmp (codecs.cpp:255-320; contract in include/icx.h) on the GPU -> (code, w, h,
        channels, uint8 (h, w, channels) or None); code is an icx_bmp_result."""
        return self._decode_image("icx_bmp_decode", BMP_INTERNAL_ERR, data, 3)

    def bmp_save_to_memory(self, px):
        """Image::writeBmp (codecs.cpp:324-375) on the GPU: uint8 (h, w) or (h, w, d), d in 1, 3, 4,
        rows top-down -> (code, the file's bytes or None)."""
        a = np.ascontiguousarray(px, np.uint8)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            return BMP_INVALID_ARGUMENT, None
        h, w, d = a.shape
        out, size = C.c_void_p(), C.c_size_t()
        code = lib().icx_bmp_save_to_memory(self._p, a.ctypes.data if a.size else None, w, h, d, C.byref(out), C.byref(size))
        if code == BMP_INTERNAL_ERR:
            raise ICXError("icx_bmp_save_to_memory: " + _err(self._p))
        if code != BMP_OK:
            return code, None
        data = C.string_at(out.value, size.value)
        lib().icx_free(out)
        return code, data

    def bmp_encode_device_batch(self, d_srcs, widths, heights, d: int, d_out: int, out_stride: int, d_sizes: int,
                                d_status: int, stream=0) -> int:
        """icx_bmp_encode_device_batch: image i's pixels at device address d_srcs[i], its file to
        d_out + i*out_stride, size (uint64) and status (int32) to the device arrays -> the call's code."""
        n = len(d_srcs)
        sp = (C.c_void_p * max(1, n))(*d_srcs)
        ws = np.ascontiguousarray(widths, np.int32)
        hs = np.ascontiguousarray(heights, np.int32)
        rc = lib().icx_bmp_encode_device_batch(self._p, n, sp, ws.ctypes.data, hs.ctypes.data, d, d_out, out_stride,
                                               d_sizes, d_status, stream or None)
        if rc == BMP_INTERNAL_ERR:
            raise ICXError("icx_bmp_encode_device_batch: " + _err(self._p))
        return rc

    def pnm_decode(self, data: bytes):
        """Image::readPbm (codecs.cpp:1034-1100; contract in include/icx.h) on the GPU -> (code, w, h,
        channels, type, maxval, array (h, w, channels) of uint8 / uint16 / float32 or None); code is an
        icx_pnm_result."""
        buf = C.create_string_buffer(bytes(data), max(1, len(data)))
        out = C.c_void_p()
        v = [C.c_int() for _ in range(5)]
        code = lib().icx_pnm_decode(self._p, buf, len(data), C.byref(out), *[C.byref(x) for x in v])
        if code == PNM_INTERNAL_ERR:
            raise ICXError("icx_pnm_decode: " + _err(self._p))
        w, h, d, t, mv = (x.value for x in v)
        arr = None
        if out.value:
            dt = np.dtype(_PNM_DTYPES[t])
            arr = np.frombuffer(C.string_at(out.value, w * h * d * dt.itemsize), dt).reshape(h, w, d).copy()
            lib().icx_free(out)
        return code, w, h, d, t, mv, arr

    def pnm_encode(self, px, fmt: int):
        """Image::writePbm (codecs.cpp:1102-1167) on the GPU: (h, w) or (h, w, d) of uint8, uint16 or
        float32, rows top-down; fmt is PNM_P4 / P5 / P6 / PF -> (code, the file's bytes or None)."""
        a = np.ascontiguousarray(px)
        if a.dtype not in (np.uint8, np.uint16, np.float32):
            return PNM_INVALID_ARGUMENT, None
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            return PNM_INVALID_ARGUMENT, None
        h, w, d = a.shape
        t = (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float32)).index(a.dtype)
        out, size = C.c_void_p(), C.c_size_t()
        code = lib().icx_pnm_save_to_memory(self._p, a.ctypes.data if a.size else None, w, h, d, t, fmt,
                                            C.byref(out), C.byref(size))
        if code == PNM_INTERNAL_ERR:
            raise ICXError("icx_pnm_save_to_memory: " + _err(self._p))
        if code != PNM_OK:
            return code, None
        data = C.string_at(out.value, size.value)
        lib().icx_free(out)
        return code, data

    def pnm_encode_device_batch(self, d_srcs, widths, heights, d: int, type_: int, fmt: int, d_out: int, out_stride: int,
                                d_sizes: int, d_status: int, stream=0) -> int:
        """icx_pnm_encode_device_batch: image i's pixels at device address d_srcs[i], its file to
        d_out + i*out_stride, size (uint64) and status (int32) to the device arrays -> the call's code."""
        n = len(d_srcs)
        sp = (C.c_void_p * max(1, n))(*d_srcs)
        ws = np.ascontiguousarray(widths, np.int32)
        hs = np.ascontiguousarray(heights, np.int32)
        rc = lib().icx_pnm_encode_device_batch(self._p, n, sp, ws.ctypes.data, hs.ctypes.data, d, type_, fmt, d_out,
                                               out_stride, d_sizes, d_status, stream or None)
        if rc == PNM_INTERNAL_ERR:
            raise ICXError("icx_pnm_encode_device_batch: " + _err(self._p))
        return rc

    def dds_decode(self, data: bytes):
        """Image::readDds (contract in include/icx.h) on the GPU: BC1-BC5, masked and copied forms ->
        (code, w, h, channels, type, array (h, w, channels) of uint8 / uint16 / float32 or None); code
        is an icx_dds_result."""
        buf = C.create_string_buffer(bytes(data), max(1, len(data)))
        out = C.c_void_p()
        v = [C.c_int() for _ in range(4)]
        code = lib().icx_dds_decode(self._p, buf, len(data), C.byref(out), *[C.byref(x) for x in v])
        if code == DDS_INTERNAL_ERR:
            raise ICXError("icx_dds_decode: " + _err(self._p))
        w, h, d, t = (x.value for x in v)
        arr = None
        if out.value:
            dt = np.dtype(_PNM_DTYPES[t])
            arr = np.frombuffer(C.string_at(out.value, w * h * d * dt.itemsize), dt).reshape(h, w, d).copy()
            lib().icx_free(out)
        return code, w, h, d, t, arr

    def dds_save_to_memory(self, px, fmt: int = DDS_RAW):
        """Image::writeDds on the GPU: uint8 (h, w) or (h, w, d), d in 1..4, rows top-down; fmt is
        DDS_RAW (uncompressed) or DDS_BC (DXT1 / DXT5 / BC4U / BC5U by d) -> (code, the file's bytes
        or None)."""
        a = np.ascontiguousarray(px)
        if a.dtype != np.uint8:
            return DDS_INVALID_ARGUMENT, None
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            return DDS_INVALID_ARGUMENT, None
        h, w, d = a.shape
        out, size = C.c_void_p(), C.c_size_t()
        code = lib().icx_dds_save_to_memory(self._p, a.ctypes.data if a.size else None, w, h, d, fmt, C.byref(out),
                                            C.byref(size))
        if code == DDS_INTERNAL_ERR:
            raise ICXError("icx_dds_save_to_memory: " + _err(self._p))
        if code != DDS_OK:
            return code, None
        data = C.string_at(out.value, size.value)
        lib().icx_free(out)
        return code, data

    def dds_encode_device_batch(self, d_srcs, widths, heights, d: int, fmt: int, d_out: int, out_stride: int, d_sizes: int,
                                d_status: int, stream=0) -> int:
        """icx_dds_encode_device_batch: image i's pixels at device address d_srcs[i], its file to
        d_out + i*out_stride, size (uint64) and status (int32) to the device arrays -> the call's code."""
        n = len(d_srcs)
        sp = (C.c_void_p * max(1, n))(*d_srcs)
        ws = np.ascontiguousarray(widths, np.int32)
        hs = np.ascontiguousarray(heights, np.int32)
        rc = lib().icx_dds_encode_device_batch(self._p, n, sp, ws.ctypes.data, hs.ctypes.data, d, fmt, d_out, out_stride,
                                               d_sizes, d_status, stream or None)
        if rc == DDS_INTERNAL_ERR:
            raise ICXError("icx_dds_encode_device_batch: " + _err(self._p))
        return rc

    def png_encode(self, width: int, height: int, d: int, src: bytes):
        """PNG bytes of an RGB8 (d=3) / RGBA8 (d=4) image (png_encoder::saveToFile), or None."""
        chunks = []

        @WRITE_FUNC
        def sink(_ctx, data, size):
            chunks.append(C.string_at(data, size))

        buf = C.create_string_buffer(bytes(src), max(1, len(src)))
        ok = lib().icx_png_encode_with_func(self._p, sink, None, buf, width, height, d)
        return b"".join(chunks) if ok == 1 else None

    def jpeg_encode(self, quality: int, subsampling: int, width: int, height: int, comps: int, src: bytes):
        """C4 extension encode (IJG quality 1..100, subsampling 444|420) -> bytes, or None."""
        chunks = []

        @WRITE_FUNC
        def sink(_ctx, data, size):
            chunks.append(C.string_at(data, size))

        buf = C.create_string_buffer(bytes(src), max(1, len(src)))
        ok = lib().icx_jpeg_encode_with_func(self._p, sink, None, quality, subsampling, width, height, comps, buf)
        return b"".join(chunks) if ok == 1 else None


class PngEncoder:
    """Device-resident PNG encode (icx_png_encoder_* / icx_png_encode_device)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._p = lib().icx_png_encoder_create(ctx.ptr)
        if not self._p:
            raise ICXError("icx_png_encoder_create failed: " + _err(ctx.ptr))

    def close(self):
        if getattr(self, "_p", None):
            lib().icx_png_encoder_destroy(self._p)
            self._p = None

    def __del__(self):
        self.close()

    def encode_device(self, width, height, d, d_src, d_out, out_cap, stream=0):
        """-> (icx_result, file size in bytes)."""
        n = C.c_uint64()
        rc = lib().icx_png_encode_device(self._p, width, height, d, d_src, d_out, out_cap, C.byref(n), stream or None)
        if rc not in (OK, OUT_OF_MEM):
            raise ICXError(f"icx_png_encode_device -> {rc}: {_err(self.ctx.ptr)}")
        return rc, int(n.value)

    def encode_device_batch(self, width, height, d, d_srcs, d_out, out_stride, stream=0):
        """n device images (list of device addresses) -> files at d_out + i*out_stride; returns
        (statuses, sizes) as numpy arrays (icx_png_encode_device_batch)."""
        n = len(d_srcs)
        srcs = (C.c_void_p * max(1, n))(*d_srcs)
        sizes = np.zeros(max(1, n), np.uint64)
        status = np.zeros(max(1, n), np.int32)
        rc = lib().icx_png_encode_device_batch(self._p, n, width, height, d, srcs, d_out, out_stride,
                                               sizes.ctypes.data, status.ctypes.data, stream or None)
        if rc != OK:
            raise ICXError(f"icx_png_encode_device_batch -> {rc}: {_err(self.ctx.ptr)}")
        return status[:n], sizes[:n].astype(np.int64)

    def stage_times(self) -> dict:
        """Summed per-stage ms since the previous call (icx_png_encoder_stage_times)."""
        names = (C.c_char_p * 8)()
        ms = (C.c_float * 8)()
        k = lib().icx_png_encoder_stage_times(self._p, names, ms, 8)
        return {names[i].decode(): float(ms[i]) for i in range(k)}


class Encoder:
    """Device-resident JPEG encode (icx_encoder_* / icx_jpeg_encode_device); pointers are device
    addresses (ints) on the context's device."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._p = lib().icx_encoder_create(ctx.ptr)
        if not self._p:
            raise ICXError("icx_encoder_create failed: " + _err(ctx.ptr))

    def close(self):
        if getattr(self, "_p", None):
            lib().icx_encoder_destroy(self._p)
            self._p = None

    def __del__(self):
        self.close()

    def encode_device(self, quality, subsampling, width, height, comps, d_src, d_out, out_cap, stream=0):
        """-> (icx_result, file size in bytes)."""
        n = C.c_uint64()
        rc = lib().icx_jpeg_encode_device(self._p, quality, subsampling, width, height, comps, d_src, d_out,
                                          out_cap, C.byref(n), stream or None)
        if rc not in (OK, OUT_OF_MEM):
            raise ICXError(f"icx_jpeg_encode_device -> {rc}: {_err(self.ctx.ptr)}")
        return rc, int(n.value)

    def encode_device_batch(self, quality, subsampling, width, height, comps, d_srcs, d_out, out_stride, stream=0):
        """n device images (list of device addresses) -> files at d_out + i*out_stride;
        returns (statuses, sizes) as numpy arrays (icx_jpeg_encode_device_batch)."""
        n = len(d_srcs)
        srcs = (C.c_void_p * max(1, n))(*d_srcs)
        sizes = np.zeros(max(1, n), np.uint64)
        status = np.zeros(max(1, n), np.int32)
        rc = lib().icx_jpeg_encode_device_batch(self._p, n, quality, subsampling, width, height, comps, srcs, d_out,
                                                out_stride, sizes.ctypes.data, status.ctypes.data, stream or None)
        if rc != OK:
            raise ICXError(f"icx_jpeg_encode_device_batch -> {rc}: {_err(self.ctx.ptr)}")
        return status[:n], sizes[:n].astype(np.int64)

    def stage_times(self) -> dict:
        """Summed per-stage ms since the previous call (icx_encoder_stage_times)."""
        names = (C.c_char_p * 8)()
        ms = (C.c_float * 8)()
        k = lib().icx_encoder_stage_times(self._p, names, ms, 8)
        return {names[i].decode(): float(ms[i]) for i in range(k)}


def probe(jpeg: bytes):
    """Host header walk (njDecode through SOS) -> (code, width, height, ncomp)."""
    w, h, n = C.c_int(), C.c_int(), C.c_int()
    buf = C.create_string_buffer(bytes(jpeg), max(1, len(jpeg)))
    code = lib().icx_jpeg_probe(buf, len(jpeg), C.byref(w), C.byref(h), C.byref(n))
    return code, w.value, h.value, n.value


def records_device(ctx: "Context", n, d_out, out_stride, d_status, d_dims, max_width, max_height, d_records,
                   stream=0):
    """icx_jpeg_records: per-image {status, w, h, ncomp, checksum64} of a batch call's outputs,
    computed on the device into d_records (n x 24 bytes, RECORD_DTYPE)."""
    rc = lib().icx_jpeg_records(ctx.ptr, n, d_out, out_stride, d_status, d_dims, max_width, max_height, d_records,
                                stream or None)
    if rc != OK:
        raise ICXError(f"icx_jpeg_records -> {rc}: {_err(ctx.ptr)}")


def checksum64(data: bytes) -> int:
    """icx_checksum64 on the host (the records' checksum of a decoded image's bytes)."""
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    return int(lib().icx_checksum64(buf, len(data)))


def multi_shard(sizes, ndev: int) -> np.ndarray:
    """icx_multi_shard: the device index each image goes to (greedy longest-first by size)."""
    n = len(sizes)
    sz = (C.c_size_t * max(1, n))(*[int(x) for x in sizes])
    out = np.zeros(max(1, n), np.int32)
    if lib().icx_multi_shard(sz, n, ndev, out.ctypes.data) != OK:
        raise ICXError("icx_multi_shard failed")
    return out[:n]


class Multi:
    """Multi-GPU decode in one process (icx_multi_*): the batch is split over `devices` by
    compressed size, one host thread per device; the records are gathered over RCCL when the
    devices are distinct (`gather` says which), the pixels copied to host memory."""

    def __init__(self, devices, max_width: int, max_height: int):
        devs = (C.c_int * len(devices))(*devices)
        self._p = lib().icx_multi_create(devs, len(devices), max_width, max_height)
        if not self._p:
            raise ICXError("icx_multi_create failed: " + _err(None))
        self.devices = list(devices)
        self.max_width, self.max_height = max_width, max_height

    @property
    def gather(self) -> str:
        return lib().icx_multi_gather(self._p).decode()

    def close(self):
        if getattr(self, "_p", None):
            lib().icx_multi_destroy(self._p)
            self._p = None

    def __del__(self):
        self.close()

    def decode_host(self, jpegs, want_pixels: bool = True):
        """-> (records (RECORD_DTYPE array), shard_of (int32 array), pixels list or None)."""
        n = len(jpegs)
        stride = self.max_width * self.max_height * 3
        bufs = [C.create_string_buffer(bytes(j), max(1, len(j))) for j in jpegs]
        ptrs = (C.c_void_p * max(1, n))(*[C.cast(b, C.c_void_p) for b in bufs])
        sizes = (C.c_size_t * max(1, n))(*[len(j) for j in jpegs])
        outs_np = [np.empty(stride, np.uint8) for _ in range(n)] if want_pixels else None
        outs = (C.c_void_p * max(1, n))(*[o.ctypes.data for o in outs_np]) if want_pixels else None
        rec = np.zeros(max(1, n), RECORD_DTYPE)
        shard_of = np.zeros(max(1, n), np.int32)
        rc = lib().icx_multi_decode_host(self._p, n, ptrs, sizes, outs, stride, rec.ctypes.data, shard_of.ctypes.data)
        if rc != OK:
            msg = lib().icx_multi_last_error(self._p)
            raise ICXError(f"icx_multi_decode_host -> {rc}: {msg.decode() if msg else ''}")
        pix = None
        if want_pixels:
            pix = []
            for i in range(n):
                r = rec[i]
                nb = int(r["width"]) * int(r["height"]) * int(r["ncomp"])
                pix.append(outs_np[i][:nb] if r["status"] == OK else None)
        return rec[:n], shard_of[:n], pix


class Batch:
    """Device-resident batched decode (icx_jpeg_batch_*). Inputs/outputs are device pointers
    (ints) -- e.g. torch CUDA tensors' data_ptr() -- on the context's device."""

    def __init__(self, ctx: Context, max_images: int, max_width: int, max_height: int, group: int = 0):
        self.ctx = ctx
        self._p = lib().icx_batch_create(ctx.ptr, max_images, max_width, max_height, group)
        if not self._p:
            raise ICXError("icx_batch_create failed: " + _err(ctx.ptr))
        self.max_images, self.max_width, self.max_height = max_images, max_width, max_height

    def close(self):
        if getattr(self, "_p", None):
            lib().icx_batch_destroy(self._p)
            self._p = None

    def __del__(self):
        self.close()

    def decode_device(self, n, d_data, d_offsets, d_sizes, d_out, out_stride, d_status, d_dims, stream=0):
        rc = lib().icx_jpeg_batch_decode(self._p, n, d_data, d_offsets, d_sizes, d_out, out_stride,
                                         d_status, d_dims, stream or None)
        if rc != OK:
            raise ICXError(f"icx_jpeg_batch_decode -> {rc}: {_err(self.ctx.ptr)}")

    def decode_host(self, jpegs, out_stride=None):
        """Decode a list of bytes objects -> list of (code, w, h, ncomp, np.ndarray|None)."""
        n = len(jpegs)
        out_stride = out_stride or self.max_width * self.max_height * 3
        bufs = [C.create_string_buffer(bytes(j), max(1, len(j))) for j in jpegs]
        ptrs = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs])
        sizes = (C.c_size_t * n)(*[len(j) for j in jpegs])
        outs_np = [np.empty(out_stride, np.uint8) for _ in range(n)]
        outs = (C.c_void_p * n)(*[o.ctypes.data for o in outs_np])
        status = np.zeros(n, np.int32)
        dims = np.zeros((n, 3), np.int32)
        rc = lib().icx_jpeg_batch_decode_host(self._p, n, ptrs, sizes, outs, out_stride,
                                              status.ctypes.data, dims.ctypes.data)
        if rc != OK:
            raise ICXError(f"icx_jpeg_batch_decode_host -> {rc}: {_err(self.ctx.ptr)}")
        res = []
        for i in range(n):
            w, h, c = (int(x) for x in dims[i])
            pix = outs_np[i][: w * h * c].reshape(h, w, c) if status[i] == OK else None
            res.append((int(status[i]), w, h, c, pix))
        return res

    def path_stats(self) -> dict:
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        lib().icx_batch_path_stats(self._p, C.byref(a), C.byref(b), C.byref(c))
        return {"parallel": a.value, "fallback": b.value, "sequential": c.value}

    def dri_stats(self) -> dict:
        """Restart-interval images of the last call planned onto the guess-write lanes: decided by
        them ("gw"), sent back to one lane per interval ("gw_fallback")."""
        a, b = C.c_int(), C.c_int()
        lib().icx_batch_dri_stats(self._p, C.byref(a), C.byref(b))
        return {"gw": a.value, "gw_fallback": b.value}

    @property
    def group(self) -> int:
        """Images per workspace group (icx_batch_group)."""
        return int(lib().icx_batch_group(self._p))

    def groups_per_call(self, n: int) -> int:
        """Groups a call of n images takes (icx_batch_groups): each per-group kernel launches once per group."""
        return int(lib().icx_batch_groups(self._p, n))

    def stage_times(self) -> dict:
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        k = lib().icx_batch_stage_times(self._p, names, ms, 16)
        return {names[i].decode(): float(ms[i]) for i in range(k)}


def hdr_probe(data: bytes):
    """Host header walk of readHdr (codecs.cpp:713-750) -> (code, width, height)."""
    w, h = C.c_int(), C.c_int()
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    code = lib().icx_hdr_probe(buf, len(data), C.byref(w), C.byref(h))
    return code, w.value, h.value


def exr_probe(data: bytes):
    """Host header / offset-table / chunk-header walk of LoadEXRFromMemory -> (code, width, height)."""
    w, h = C.c_int(), C.c_int()
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    code = lib().icx_exr_probe(buf, len(data), C.byref(w), C.byref(h))
    return code, w.value, h.value


def hdr_encode_bound(width: int, height: int, d: int, rle: bool = False) -> int:
    """icx_hdr_encode_bound: the largest file the write can give, or 0 for arguments it refuses."""
    return int(lib().icx_hdr_encode_bound(width, height, d, 1 if rle else 0))


def tga_probe(data: bytes):
    """Host header walk of the Targa read -> (code, width, height, channels)."""
    w, h, d = C.c_int(), C.c_int(), C.c_int()
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    code = lib().icx_tga_probe(buf, len(data), C.byref(w), C.byref(h), C.byref(d))
    return code, w.value, h.value, d.value


def bmp_probe(data: bytes):
    """Host header walk of the BMP read -> (code, width, height, channels)."""
    w, h, d = C.c_int(), C.c_int(), C.c_int()
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    code = lib().icx_bmp_probe(buf, len(data), C.byref(w), C.byref(h), C.byref(d))
    return code, w.value, h.value, d.value


def bmp_encode_bound(width: int, height: int, d: int) -> int:
    """icx_bmp_encode_bound: the written file's size, or 0 for arguments the write refuses."""
    return int(lib().icx_bmp_encode_bound(width, height, d))


def gif_probe(data: bytes):
    """Host container walk of the GIF read, up to the first image descriptor -> (code, width, height)."""
    w, h = C.c_int(), C.c_int()
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    code = lib().icx_gif_probe(buf, len(data), C.byref(w), C.byref(h))
    return code, w.value, h.value


def tiff_probe(data: bytes):
    """Host IFD walk of the TIFF read -> (code, width, height, channels)."""
    w, h, d = C.c_int(), C.c_int(), C.c_int()
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    code = lib().icx_tiff_probe(buf, len(data), C.byref(w), C.byref(h), C.byref(d))
    return code, w.value, h.value, d.value


def gif_encode_bound(width: int, height: int, segment_pixels: int = 0) -> int:
    """icx_gif_encode_bound: an upper bound of the written file's size, or 0 for arguments the
    write refuses."""
    return int(lib().icx_gif_encode_bound(width, height, segment_pixels))


def tiff_encode_bound(width: int, height: int, d: int, compression: int = TIFF_COMPRESSION_DEFLATE, predictor: int = 1,
                      rows_per_strip: int = 0) -> int:
    """icx_tiff_encode_bound: an upper bound of the written file's size, or 0 for arguments the
    write refuses."""
    return int(lib().icx_tiff_encode_bound(width, height, d, compression, predictor, rows_per_strip))


def tga_encode_bound(width: int, height: int, d: int) -> int:
    """icx_tga_encode_bound: 18 + w*h*(d+1), or 0 for arguments the write refuses."""
    return int(lib().icx_tga_encode_bound(width, height, d))


def pnm_probe(data: bytes):
    """Host header walk of the Netpbm read -> (code, width, height, channels, type, maxval)."""
    v = [C.c_int() for _ in range(5)]
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    code = lib().icx_pnm_probe(buf, len(data), *[C.byref(x) for x in v])
    return (code, *(x.value for x in v))


def pnm_encode_bound(width: int, height: int, d: int, type_: int, fmt: int) -> int:
    """icx_pnm_encode_bound: the file's length, or 0 for arguments the write refuses."""
    return int(lib().icx_pnm_encode_bound(width, height, d, type_, fmt))


def dds_probe(data: bytes):
    """Host header walk of the DDS read -> (code, width, height, channels, type)."""
    v = [C.c_int() for _ in range(4)]
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    code = lib().icx_dds_probe(buf, len(data), *[C.byref(x) for x in v])
    return (code, *(x.value for x in v))


def dds_encode_bound(width: int, height: int, d: int, fmt: int) -> int:
    """icx_dds_encode_bound: the file's length, or 0 for arguments the write refuses."""
    return int(lib().icx_dds_encode_bound(width, height, d, fmt))


class _ReadBatch:
    """What the read batches share (icx_<fmt>_batch_*); a subclass names its entries and codes."""

    _prefix = ""    # the entries are <_prefix>_create, _destroy, _decode, _stage_times
    _ok = 0
    _returned = ()  # codes besides _ok that _decode returns instead of raising

    def __init__(self, ctx: Context, max_images: int, max_width: int, max_height: int):
        self.ctx = ctx
        self._p = self._entry("create")(ctx.ptr, max_images, max_width, max_height)
        if not self._p:
            raise ICXError(f"{self._prefix}_create failed: " + _err(ctx.ptr))
        self.max_images, self.max_width, self.max_height = max_images, max_width, max_height

    def _entry(self, name: str):
        return getattr(lib(), f"{self._prefix}_{name}")

    def close(self):
        if getattr(self, "_p", None):
            self._entry("destroy")(self._p)
            self._p = None

    def __del__(self):
        self.close()

    def _decode(self, n, d_data, d_offsets, d_sizes, d_out, out_stride, d_status, d_dims, stream=0) -> int:
        rc = self._entry("decode")(self._p, n, d_data, d_offsets, d_sizes, d_out, out_stride, d_status, d_dims,
                                   stream or None)
        if rc != self._ok and rc not in self._returned:
            raise ICXError(f"{self._prefix}_decode -> {rc}: {_err(self.ctx.ptr)}")
        return rc

    def decode_device(self, n, d_data, d_offsets, d_sizes, d_out, out_stride, d_status, d_dims, stream=0):
        self._decode(n, d_data, d_offsets, d_sizes, d_out, out_stride, d_status, d_dims, stream)

    def stage_times(self) -> dict:
        names = (C.c_char_p * 8)()
        ms = (C.c_float * 8)()
        k = self._entry("stage_times")(self._p, names, ms, 8)
        return {names[i].decode(): float(ms[i]) for i in range(k)}


class PnmBatch(_ReadBatch):
    """Device-resident batched Netpbm decode (icx_pnm_batch_*): image i is
    d_data[d_offsets[i] .. + d_sizes[i]); its elements at d_out + i*out_stride (d_out 16-byte aligned,
    out_stride a multiple of 16), status in d_status[i], {width, height, channels, type, maxval} in
    d_dims[5i..]."""

    _prefix, _ok, _returned = "icx_pnm_batch", PNM_OK, (PNM_INVALID_ARGUMENT,)

    def decode_device(self, n, d_data, d_offsets, d_sizes, d_out, out_stride, d_status, d_dims, stream=0) -> int:
        """-> PNM_OK, or PNM_INVALID_ARGUMENT for a d_out or out_stride that is not 16-byte aligned."""
        return self._decode(n, d_data, d_offsets, d_sizes, d_out, out_stride, d_status, d_dims, stream)


class DdsBatch(_ReadBatch):
    """Device-resident batched DDS decode (icx_dds_batch_*): image i is
    d_data[d_offsets[i] .. + d_sizes[i]); its elements at d_out + i*out_stride (d_out 16-byte aligned,
    out_stride a multiple of 16), status in d_status[i], {width, height, channels, type} in
    d_dims[4i..]."""

    _prefix, _ok, _returned = "icx_dds_batch", DDS_OK, (DDS_INVALID_ARGUMENT,)

    def decode_device(self, n, d_data, d_offsets, d_sizes, d_out, out_stride, d_status, d_dims, stream=0) -> int:
        """-> DDS_OK, or DDS_INVALID_ARGUMENT for a d_out or out_stride that is not 16-byte aligned."""
        return self._decode(n, d_data, d_offsets, d_sizes, d_out, out_stride, d_status, d_dims, stream)


def png_probe(data: bytes):
    """Host chunk walk of the PNG read (signature, IHDR, PLTE / tRNS, IDAT present) -> (code, width, height)."""
    w, h = C.c_int(), C.c_int()
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    code = lib().icx_png_probe(buf, len(data), C.byref(w), C.byref(h))
    return code, w.value, h.value


class PngBatch(_ReadBatch):
    """Device-resident batched PNG decode (icx_png_batch_*): image i is
    d_data[d_offsets[i] .. + d_sizes[i]); RGBA8 at d_out + i*out_stride bytes, status in
    d_status[i], {width, height, 4} in d_dims[3i..]."""

    _prefix, _ok = "icx_png_batch", PNGR_OK


class TgaBatch(_ReadBatch):
    """Device-resident batched Targa decode (icx_tga_batch_*): image i is
    d_data[d_offsets[i] .. + d_sizes[i]); its bytes at d_out + i*out_stride, status in d_status[i],
    {width, height, channels} in d_dims[3i..]."""

    _prefix, _ok = "icx_tga_batch", TGA_OK


class BmpBatch(_ReadBatch):
    """Device-resident batched BMP decode (icx_bmp_batch_*): image i is
    d_data[d_offsets[i] .. + d_sizes[i]); its bytes at d_out + i*out_stride, status in d_status[i],
    {width, height, channels} in d_dims[3i..]."""

    _prefix, _ok = "icx_bmp_batch", BMP_OK


class GifBatch(_ReadBatch):
    """Device-resident batched GIF decode (icx_gif_batch_*): image i is
    d_data[d_offsets[i] .. + d_sizes[i]); its R,G,B bytes at d_out + i*out_stride, status in
    d_status[i], {width, height, 3} in d_dims[3i..]."""

    _prefix, _ok = "icx_gif_batch", GIF_OK


class TiffBatch(_ReadBatch):
    """Device-resident batched TIFF decode (icx_tiff_batch_*): image i is
    d_data[d_offsets[i] .. + d_sizes[i]); its bytes at d_out + i*out_stride
    (out_stride >= 4 * max_width * max_height), status in
    d_status[i], {width, height, channels} in d_dims[3i..]."""

    _prefix, _ok = "icx_tiff_batch", TIFF_OK


class HdrBatch(_ReadBatch):
    """Device-resident batched Radiance .hdr decode (icx_hdr_batch_*): image i is
    d_data[d_offsets[i] .. + d_sizes[i]); 4 floats per pixel at d_out + i*out_stride floats."""

    _prefix, _ok = "icx_hdr_batch", HDR_OK

    def locate_stats(self) -> list:
        """icx_hdr_batch_locate_stats: (mode, ncand) of each image of the last decode -- mode 0 failed
        before locating, 1 all rows plain, 2 scanline starts linked in parallel, 3 walked serially;
        ncand the new-style scanline start patterns found. Waits for that decode's work."""
        cap = self.max_images
        modes, ncand = (C.c_int32 * cap)(), (C.c_int32 * cap)()
        n = lib().icx_hdr_batch_locate_stats(self._p, modes, ncand, cap)
        if n < 0:
            raise ICXError("icx_hdr_batch_locate_stats: " + _err(self.ctx.ptr))
        return [(int(modes[i]), int(ncand[i])) for i in range(n)]


class Image:
    """ImageCodecs::Image (codecs.h:16-103) for the JPEG hot path.

    read()/write() dispatch on the lower-cased extension like Image::read/write
    (codecs.cpp:53-122): read .jpg/.jpeg (readJpg), .png (readPng: d = 4, type UBYTE) and .hdr
    (readHdr: d = 4, type FLOAT, the floats' bytes in pixels_), .exr, .tga (readTga: d = 1, 3 or
    4, type UBYTE), .gif (readGif: the first frame, d = 3, type UBYTE) and .tif/.tiff (readTiff: d = 1,
    3 or 4, type UBYTE), write .jpg/.jpeg, .png, .exr,
    .tga (uncompressed) and .hdr (flat RGBE; d = 4 only). .bmp is read (readBmp: d = 1, 3 or 4, type
    UBYTE; raw, RLE4 / RLE8 and bitfields files) and written (writeBmp: 8-bit grey, 24-bit or 32-bit). .pbm/.pgm/.ppm/.pnm/.pfm are read by
    their magic (readPbm: d = 1 or 3; UBYTE, USHORT or FLOAT) and written as P4 / P5 / P6 / P5 or P6
    by d / PF or Pf (writePbm). .dds is read (readDds: BC1-BC5 decoded, masked and copied forms; d = 1..4; UBYTE,
    USHORT or FLOAT) and written uncompressed (writeDds; UBYTE only). Other extensions raise ValueError (the reference's
    std::invalid_argument for unknown types)."""

    _PNM_EXT = (".pbm", ".pgm", ".ppm", ".pnm", ".pfm")

    UBYTE, USHORT, FLOAT = range(3)  # ImageCodecs::Type (codecs.h:14)
    _ctx = None

    def __init__(self):
        self.h_ = self.w_ = self.d_ = 0
        self.pixels_ = None
        self.type_ = Image.UBYTE

    @classmethod
    def context(cls):
        if cls._ctx is None:
            cls._ctx = Context(0)
        return cls._ctx

    def read(self, filepath: str):
        ext = os.path.splitext(filepath)[1].lower()
        if ext == ".hdr":
            self._read_hdr(filepath)
            return
        if ext == ".exr":
            self._read_exr(filepath)
            return
        if ext == ".png":
            self._read_png(filepath)
            return
        if ext == ".tga":
            self._read_tga(filepath)
            return
        if ext == ".bmp":
            self._read_bmp(filepath)
            return
        if ext == ".gif":
            self._read_gif(filepath)
            return
        if ext in (".tif", ".tiff"):
            self._read_tiff(filepath)
            return
        if ext in Image._PNM_EXT:
            self._read_pnm(filepath)
            return
        if ext == ".dds":
            self._read_dds(filepath)
            return
        if ext not in (".jpg", ".jpeg"):
            raise ValueError("Cannot parse filetype")
        data = open(filepath, "rb").read()
        code, w, h, n, pix = self.context().decode(data)
        if code != OK:
            raise RuntimeError("Error decoding the input file.\n")  # codecs.cpp:836
        self.w_, self.h_, self.d_ = w, h, n
        self.pixels_ = np.frombuffer(pix, np.uint8).copy()
        self.type_ = Image.UBYTE

    def _read_hdr(self, filepath: str):
        """readHdr (codecs.cpp:706-777). A truncated file keeps its decoded rows (the rest are
        zero; the reference leaves them uninitialised); header errors and run-length data the
        reference cannot decode raise RuntimeError("Invalid file format") (:732, :748)."""
        data = open(filepath, "rb").read()
        code, w, h, rows, px = self.context().hdr_decode(data)
        if code not in (HDR_OK, HDR_TRUNCATED):
            raise RuntimeError("Invalid file format")
        self.w_, self.h_, self.d_ = w, h, 4
        self.pixels_ = px.reshape(-1).view(np.uint8).copy()
        self.type_ = Image.FLOAT

    def _read_bytes(self, decode, ok: int, filepath: str, d=None):
        """The byte readers' body: decode(file) -> (code, w, h[, d], pixels); d where the format fixes it."""
        code, w, h, *dd, px = decode(open(filepath, "rb").read())
        if code != ok:
            raise RuntimeError("Could not read image data")
        self.w_, self.h_, self.d_ = w, h, d or dd[0]
        self.pixels_ = px.reshape(-1).copy()
        self.type_ = Image.UBYTE

    def _read_png(self, filepath: str):
        """readPng (codecs.cpp:903-1020): d = 4, type UBYTE, 8-bit RGBA rows top-down. Every
        failure is Image::read's RuntimeError("Could not read image data") (:85-88: readPng leaves
        pixels_ null)."""
        self._read_bytes(self.context().png_decode, PNGR_OK, filepath, 4)

    def _read_tga(self, filepath: str):
        """readTga (codecs.cpp:1304-1407): d = 1, 3 or 4, type UBYTE, rows top-down. Every failure is
        Image::read's RuntimeError("Could not read image data") (:85-88: pixels_ stays null)."""
        self._read_bytes(self.context().tga_decode, TGA_OK, filepath)

    def _read_bmp(self, filepath: str):
        """readBmp (codecs.cpp:255-320): d = 1, 3 or 4, type UBYTE, rows top-down. Every failure is
        Image::read's RuntimeError("Could not read image data") (:85-88: pixels_ stays null)."""
        self._read_bytes(self.context().bmp_decode, BMP_OK, filepath)

    def _read_gif(self, filepath: str):
        """readGif (codecs.cpp:507-542): the first frame on the logical screen, d = 3, type UBYTE,
        rows top-down. Every failure is Image::read's RuntimeError("Could not read image data")."""
        self._read_bytes(self.context().gif_decode, GIF_OK, filepath, 3)

    def _read_tiff(self, filepath: str):
        """readTiff (codecs.cpp:1439-1484): the first IFD, d = 1, 3 or 4, type UBYTE, rows top-down.
        Every failure is Image::read's RuntimeError("Could not read image data")."""
        self._read_bytes(self.context().tiff_decode, TIFF_OK, filepath)

    def _read_pnm(self, filepath: str):
        """readPbm (codecs.cpp:1034-1100): the type is the magic's, whatever the name; d = 1 or 3, type
        UBYTE, USHORT or FLOAT, rows top-down. Every failure is Image::read's RuntimeError("Could not
        read image data")."""
        data = open(filepath, "rb").read()
        code, w, h, d, t, _, px = self.context().pnm_decode(data)
        if code != PNM_OK:
            raise RuntimeError("Could not read image data")
        self.w_, self.h_, self.d_ = w, h, d
        self.pixels_ = px.reshape(-1).view(np.uint8).copy()
        self.type_ = t

    def _read_dds(self, filepath: str):
        """readDds (contract in include/icx.h): BC1-BC5 decoded, masked and copied forms; d = 1..4, type
        UBYTE, USHORT or FLOAT, rows top-down. Every failure is Image::read's RuntimeError("Could not
        read image data")."""
        code, w, h, d, t, px = self.context().dds_decode(open(filepath, "rb").read())
        if code != DDS_OK:
            raise RuntimeError("Could not read image data")
        self.w_, self.h_, self.d_ = w, h, d
        self.pixels_ = px.reshape(-1).view(np.uint8).copy()
        self.type_ = t

    def _read_exr(self, filepath: str):
        """readExr (codecs.cpp:464-493): LoadEXRFromMemory -> d = 4, type FLOAT, the floats' bytes in
        pixels_; a failure raises RuntimeError("Could not load .exr") (:489). (The reference reads
        the file with a loop that appends one extra byte, ifile.get()'s EOF, :468-471; tinyexr
        ignores bytes past the last chunk, so the result is the same.)"""
        data = open(filepath, "rb").read()
        code, w, h, px = self.context().exr_decode(data + b"\xff")
        if code != EXR_SUCCESS:
            raise RuntimeError("Could not load .exr")
        self.w_, self.h_, self.d_ = w, h, 4
        self.pixels_ = px.reshape(-1).view(np.uint8).copy()
        self.type_ = Image.FLOAT

    def write(self, filepath: str):
        ext = os.path.splitext(filepath)[1].lower()
        if ext == ".png":  # writePng -> png_encoder::saveToFile (codecs.cpp:1022-1025)
            out = self.context().png_encode(self.w_, self.h_, self.d_, self.pixels_.tobytes())
        elif ext in (".jpg", ".jpeg"):
            out = self.context().tje_encode(3, self.w_, self.h_, self.d_, self.pixels_.tobytes())  # codecs.cpp:853
        elif ext == ".exr":  # writeExr -> SaveEXR(float*, w, h, d, fp16 = 0) (codecs.cpp:495-505)
            try:  # (the reference only prints tinyexr's message: nothing is thrown, no file appears)
                px = np.frombuffer(self.pixels_.tobytes(), np.float32, self.w_ * self.h_ * self.d_)
                out = self.context().exr_encode(px.reshape(self.h_, self.w_, self.d_))
            except (ICXError, ValueError):
                return
        elif ext == ".tga":  # writeTga (codecs.cpp:1410-1437): uncompressed; nothing is thrown on failure
            try:
                px = np.frombuffer(self.pixels_.tobytes(), np.uint8, self.w_ * self.h_ * self.d_)
                code, out = self.context().tga_encode(px.reshape(self.h_, self.w_, self.d_))
            except (ICXError, ValueError, AttributeError):
                return
            if code != TGA_OK:
                return
        elif ext == ".bmp":  # writeBmp (codecs.cpp:324-375): nothing is thrown on failure
            try:
                px = np.frombuffer(self.pixels_.tobytes(), np.uint8, self.w_ * self.h_ * self.d_)
                code, out = self.context().bmp_save_to_memory(px.reshape(self.h_, self.w_, self.d_))
            except (ICXError, ValueError, AttributeError):
                return
            if code != BMP_OK:
                return
        elif ext == ".dds":  # writeDds: uncompressed, UBYTE only; nothing is thrown on failure
            if self.type_ != Image.UBYTE:
                return
            try:
                px = np.frombuffer(self.pixels_.tobytes(), np.uint8, self.w_ * self.h_ * self.d_)
                code, out = self.context().dds_save_to_memory(px.reshape(self.h_, self.w_, self.d_), DDS_RAW)
            except (ICXError, ValueError, AttributeError):
                return
            if code != DDS_OK:
                return
        elif ext == ".hdr":  # writeHdr (codecs.cpp:779-818): flat RGBE; d != 4 throws (:781-784)
            if self.d_ != 4:
                raise RuntimeError("HDR data must contain a 4th channel of exposure values")
            try:  # (type_ is not consulted: pixels_ is read as floats, as for .exr)
                px = np.frombuffer(self.pixels_.tobytes(), np.float32, self.w_ * self.h_ * 4)
                code, out = self.context().hdr_encode(px.reshape(self.h_, self.w_, 4))
            except (ICXError, ValueError, AttributeError):
                return
            if code != HDR_OK:
                return
        elif ext in Image._PNM_EXT:  # writePbm (codecs.cpp:1102-1167)
            if ext == ".pfm" and self.type_ != Image.FLOAT:
                raise RuntimeError("Cannot write non-float data to .pfm")  # :1149-1152
            fmt = {".pbm": PNM_P4, ".pgm": PNM_P5, ".ppm": PNM_P6, ".pfm": PNM_PF}.get(ext, PNM_P5 if self.d_ == 1 else PNM_P6)
            try:  # (every other failure: nothing is thrown, no file appears)
                px = np.frombuffer(self.pixels_.tobytes(), _PNM_DTYPES[self.type_], self.w_ * self.h_ * self.d_)
                code, out = self.context().pnm_encode(px.reshape(self.h_, self.w_, self.d_), fmt)
            except (ICXError, ValueError, AttributeError):
                return
            if code != PNM_OK:
                return
        else:
            raise ValueError("Cannot parse filetype")
        with open(filepath, "wb") as f:
            if out is not None:
                f.write(out)

    def writeTiff(self, filepath: str, compression: int = TIFF_COMPRESSION_DEFLATE, predictor: int = 1,
                  rows_per_strip: int = 0):
        """writeTiff (private in the reference, codecs.cpp:1485-1513) called by name, whatever the
        path's extension; write(".tif") does not dispatch to it yet. UBYTE only. Nothing is thrown:
        a failure prints a line and writes nothing."""
        if self.type_ != Image.UBYTE:
            print("writeTiff: only UBYTE images are written", file=sys.stderr)
            return
        try:
            px = np.frombuffer(self.pixels_.tobytes(), np.uint8, self.w_ * self.h_ * self.d_)
            code, out = self.context().tiff_save_to_memory(px.reshape(self.h_, self.w_, self.d_), compression, predictor,
                                                           rows_per_strip)
        except (ICXError, ValueError, AttributeError) as e:
            print("writeTiff:", e, file=sys.stderr)
            return
        if code != TIFF_OK:
            print("icx_tiff_save_to_memory ->", code, file=sys.stderr)
            return
        with open(filepath, "wb") as f:
            f.write(out)

    def writeGif(self, filepath: str, segment_pixels: int = 0, dither: bool = False):
        """writeGif (private in the reference, codecs.cpp:544-594) called by name, whatever the
        path's extension; write(".gif") does not dispatch to it. UBYTE only. Nothing is thrown: a
        failure prints a line and writes nothing."""
        if self.type_ != Image.UBYTE:
            print("writeGif: only UBYTE images are written", file=sys.stderr)
            return
        try:
            px = np.frombuffer(self.pixels_.tobytes(), np.uint8, self.w_ * self.h_ * self.d_)
            code, out = self.context().gif_save_to_memory(px.reshape(self.h_, self.w_, self.d_), segment_pixels, dither)
        except (ICXError, ValueError, AttributeError) as e:
            print("writeGif:", e, file=sys.stderr)
            return
        if code != GIF_OK:
            print("icx_gif_save_to_memory ->", code, file=sys.stderr)
            return
        with open(filepath, "wb") as f:
            f.write(out)

    def load(self, pixels, w: int, h: int, channels: int, type_: int = None):
        """load(pixels, w, h, channels): UBYTE, as the reference's. With a fifth argument the pixels
        are w*h*channels elements of that type (uint8, uint16 or float32), kept as their bytes."""
        if type_ is None:
            self.pixels_ = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
            type_ = Image.UBYTE
        else:
            self.pixels_ = np.ascontiguousarray(pixels, _PNM_DTYPES[type_]).reshape(-1).view(np.uint8)
        self.w_, self.h_, self.d_ = w, h, channels
        self.type_ = type_

    def rows(self):
        return self.h_

    def cols(self):
        return self.w_

    def channels(self):
        return self.d_

    def empty(self):
        return self.h_ == 0 or self.w_ == 0 or self.d_ == 0 or self.pixels_ is None

    def byteSize(self):
        return 4 if self.type_ == Image.FLOAT else 2 if self.type_ == Image.USHORT else 1

    def type(self):
        return self.type_

    def totalBytes(self):
        return self.w_ * self.h_ * self.d_ * self.byteSize()

    def data(self):
        return self.pixels_
