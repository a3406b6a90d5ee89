"""CPU-side checks of the Radiance .hdr write's C ABI: the four entries are exported and bound,
icx_hdr_encode_bound's values, refused arguments answered without a device, and no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
import imagecodecs_amd as icx
import hdrwutil as U

ENTRIES = ("icx_hdr_encode_bound", "icx_hdr_save_to_memory", "icx_hdr_save_to_file", "icx_hdr_encode_device_batch")


def test_exported_and_bound():
    icx.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", icx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icx_\w+)", out))
    for name in ENTRIES:
        assert name in exported and name in icx._SIGS, name
    src = open(os.path.join(ROOT, "include", "icx.h")).read()
    assert "ICX_HDR_INVALID_ARGUMENT = 6," in src and "ICX_HDR_TOO_LARGE = 5," in src
    assert icx.HDR_INVALID_ARGUMENT == U.INVALID_ARGUMENT == 6 and icx.HDR_TOO_LARGE == U.TOO_LARGE == 5


def test_encode_bound():
    assert icx.hdr_encode_bound(499, 289, 4, False) == len(U.header(499, 289)) + 4 * 499 * 289
    assert icx.hdr_encode_bound(499, 289, 3, True) == len(U.header(499, 289)) + 289 * (4 + 4 * (499 + 4))
    assert icx.hdr_encode_bound(4096, 4096, 4, False) == 65 + 4 * 4096 * 4096
    for w, h, d, rle in ((1, 1, 4, True), (7, 3, 3, True), (8, 3, 3, True), (128, 2, 4, True), (129, 2, 4, True),
                         (32767, 2, 4, True), (32768, 2, 4, True), (1 << 30, 1, 3, False), (1, 1 << 30, 4, True)):
        assert icx.hdr_encode_bound(w, h, d, rle) == U.encode_bound(w, h, d, rle) > 0, (w, h, d, rle)
    for w, h, d in ((0, 4, 4), (4, 0, 4), (-1, 4, 4), (4, -1, 3), (4, 4, 1), (4, 4, 2), (4, 4, 5), ((1 << 30) + 1, 1, 4),
                    (1 << 15, (1 << 15) + 1, 4)):
        assert icx.hdr_encode_bound(w, h, d, False) == icx.hdr_encode_bound(w, h, d, True) == 0, (w, h, d)


def test_refused_arguments_need_no_device():
    """Bad arguments are answered before the context is looked at: a null context serves."""
    L = icx.lib()
    a = np.ones((4, 4, 4), np.float32)
    out, size = C.c_void_p(), C.c_size_t(5)
    for w, h, d in ((4, 4, 2), (0, 4, 4), (4, 0, 4), (4, 4, 5), (-3, 4, 3)):
        assert L.icx_hdr_save_to_memory(None, a.ctypes.data, w, h, d, 0, C.byref(out), C.byref(size)) == icx.HDR_INVALID_ARGUMENT
        assert out.value is None and size.value == 0
    assert L.icx_hdr_save_to_memory(None, None, 4, 4, 4, 0, C.byref(out), C.byref(size)) == icx.HDR_INVALID_ARGUMENT
    assert L.icx_hdr_save_to_memory(None, a.ctypes.data, 4, 4, 4, 0, None, C.byref(size)) == icx.HDR_INVALID_ARGUMENT
    assert L.icx_hdr_save_to_file(None, None, a.ctypes.data, 4, 4, 4, 0) == icx.HDR_INVALID_ARGUMENT
    assert L.icx_hdr_save_to_file(None, b"/nonexistent/x.hdr", a.ctypes.data, 4, 4, 7, 0) == icx.HDR_INVALID_ARGUMENT
    assert L.icx_hdr_encode_device_batch(None, 1, None, None, None, 4, 0, None, 0, None, None, None) == icx.HDR_INVALID_ARGUMENT
    assert L.icx_hdr_encode_device_batch(None, 0, None, None, None, 2, 0, None, 0, None, None, None) == icx.HDR_INVALID_ARGUMENT
    assert L.icx_hdr_encode_device_batch(None, -1, None, None, None, 4, 0, None, 0, None, None, None) == icx.HDR_INVALID_ARGUMENT


def test_no_cpu_fallback_without_gpu():
    """Without a GPU there is no context; the write reports ICX_HDR_INTERNAL_ERR and the reason is
    the context's "no HIP device" (as the other writes do). With a GPU this is test_gpu_hdr_write's."""
    import torch
    if torch.cuda.is_available():
        return
    L = icx.lib()
    assert L.icx_create(0) is None
    a = np.ones((4, 4, 4), np.float32)
    out, size = C.c_void_p(), C.c_size_t()
    assert L.icx_hdr_save_to_memory(None, a.ctypes.data, 4, 4, 4, 0, C.byref(out), C.byref(size)) == icx.HDR_INTERNAL_ERR
    assert out.value is None and b"no HIP device" in L.icx_last_error(None)
    assert L.icx_hdr_save_to_file(None, b"x.hdr", a.ctypes.data, 4, 4, 4, 1) == icx.HDR_INTERNAL_ERR
    try:
        icx.Context(0)
    except icx.ICXError as e:
        assert "no HIP device" in str(e)
    else:
        raise AssertionError("Context(0) without a GPU")
