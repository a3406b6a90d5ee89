"""The host layer the seven read batches share (hdr, png, tga, bmp, pnm, gif, tiff): what each
entry refuses, in which order and with which code and message, and that a one-shot decode and a
batch of one agree.

The kernels' results are pinned by test_gpu_<fmt>.py; this file pins the argument checks and
error paths around them, format by format, where the formats differ on purpose: the limits
batch_create refuses, the order of batch_decode's checks, the out_stride floor (4 x w x h, 3 for
gif, none for pnm), the alignment png and pnm ask for, the stage names, and which workspace the
one-shot builds (tga / bmp / pnm with and without tile tables, tiff at the padded size). Every
image is at most 16 x 16 and every batch holds at most 3."""
import ctypes as C

import numpy as np
import pytest

import bmputil as B
import gifutil as G
import hdrutil as H
import imagecodecs_amd as icx
import pngread_util as PR
import pnmutil as P
import tgautil as T
import tiffutil as TF
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
W, H_ = 5, 3     # the files
MW, MH = 16, 16  # the batches that decode them (the tiled tiff's padded size)
LIMIT = 1 << 30  # pixels


def _gif_file():
    idx = np.random.default_rng(3).integers(0, 4, (H_, W), dtype=np.uint8)
    return G.simple_gif(idx, G.palette(4))


def _bmp_rle8():
    return B.rle_file(8, W, H_, b"".join(B.run(W, y + 1) + B.EOL for y in range(H_)) + B.EOB)


def _pnm_p2():
    px = P.synth(2, W, H_, 1)
    return P.text_file(b"2", W, H_, 255, P.text_of(px), [b" ", b"\n"])


# per format: the batch class, codes, the stride floor per pixel, bytes per stride unit, ints per
# image in d_dims, the stage names in order, sizes batch_create refuses beyond non-positive ones and
# sizes at the edge it accepts, the one-shot's workspace variants, the probe
_COMMON_BAD = [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)]
_PIXELS_BAD = [(1, 32769, 32768)]  # one pixel row above 2^30
SPEC = {
    "hdr": dict(cls=icx.HdrBatch, ok=icx.HDR_OK, internal=icx.HDR_INTERNAL_ERR, floor=4, unit=4, ndims=3,
                stages=["parse", "locate", "unpack", "convert"], bad=[], good=[(65536, 1, 1)],
                files=lambda: {"flat": H.S.hdr(H.S.rgbe(1, W, H_), H.FLAT)}, probe=icx.hdr_probe),
    "png": dict(cls=icx.PngBatch, ok=icx.PNGR_OK, internal=icx.PNGR_INTERNAL_ERR, floor=4, unit=1, ndims=3,
                stages=["parse", "gather", "inflate", "unfilter", "expand"],
                bad=[(65536, 1, 1), (1, 0x1000001, 1), (1, 1, 0x1000001)], good=[(65535, 1, 1)],
                files=lambda: {"rgb8": PR.make_png(PR.random_samples(np.random.default_rng(4), W, H_, 8, 2), 8, 2)},
                probe=icx.png_probe),
    "tga": dict(cls=icx.TgaBatch, ok=icx.TGA_OK, internal=icx.TGA_INTERNAL_ERR, floor=4, unit=1, ndims=3,
                stages=["parse", "locate", "expand", "raw"],
                bad=[(65536, 1, 1), (1, 65536, 1), (1, 1, 65536)] + _PIXELS_BAD,
                good=[(65535, 1, 1), (1, 65535, 1), (1, 1, 65535)],
                files=lambda: {"raw": T.tga_file(T.synth(5, W, H_, 3)), "rle": T.tga_file(T.synth(5, W, H_, 3), rle=True)},
                probe=icx.tga_probe),
    "bmp": dict(cls=icx.BmpBatch, ok=icx.BMP_OK, internal=icx.BMP_INTERNAL_ERR, floor=4, unit=1, ndims=3,
                stages=["parse", "locate", "fill", "expand", "raw"],
                bad=[(65536, 1, 1)] + _PIXELS_BAD, good=[(65535, 1, 1), (1, 65536, 1)],
                files=lambda: {"raw": B.raw_file(6, 24, W, H_), "rle8": _bmp_rle8()}, probe=icx.bmp_probe),
    "pnm": dict(cls=icx.PnmBatch, ok=icx.PNM_OK, internal=icx.PNM_INTERNAL_ERR, floor=0, unit=1, ndims=5,
                stages=["parse", "locate", "text", "stream"],
                bad=[(65536, 1, 1)] + _PIXELS_BAD, good=[(65535, 1, 1), (1, 65536, 1)],
                files=lambda: {"p5": P.binary_file(P.synth(7, W, H_, 1)), "p2": _pnm_p2()}, probe=icx.pnm_probe),
    "gif": dict(cls=icx.GifBatch, ok=icx.GIF_OK, internal=icx.GIF_INTERNAL_ERR, floor=3, unit=1, ndims=3,
                stages=["parse", "lzw", "render"],
                bad=[(65536, 1, 1), (1, 65536, 1), (1, 1, 65536)] + _PIXELS_BAD,
                good=[(65535, 1, 1), (1, 65535, 1), (1, 1, 65535)],
                files=lambda: {"gif": _gif_file()}, probe=icx.gif_probe),
    "tiff": dict(cls=icx.TiffBatch, ok=icx.TIFF_OK, internal=icx.TIFF_INTERNAL_ERR, floor=4, unit=1, ndims=3,
                 stages=["parse", "unpack", "render"],
                 bad=[(65536, 1, 1)] + _PIXELS_BAD, good=[(65535, 1, 1), (1, 65536, 1)],
                 files=lambda: {"strip": TF.make_tiff(TF.noise(8, H_, W, 3)),
                                "tiled": TF.make_tiff(TF.noise(8, H_, W, 3), tile=(MW, MH))},
                 probe=icx.tiff_probe),
}
FMTS = list(SPEC)
VARIANTS = [(f, v) for f in FMTS for v in {"hdr": ["flat"], "png": ["rgb8"], "tga": ["raw", "rle"], "bmp": ["raw", "rle8"],
                                            "pnm": ["p5", "p2"], "gif": ["gif"], "tiff": ["strip", "tiled"]}[f]]


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files():
    return {f: SPEC[f]["files"]() for f in FMTS}


def _err(ctx):
    return icx.lib().icx_last_error(ctx.ptr).decode()


def _dirty(ctx):
    """Leaves another entry's message in the context, so that a message read next is a new one."""
    assert not icx.lib().icx_batch_create(ctx.ptr, 0, 1, 1, 1)
    assert _err(ctx) == "icx_batch_create: bad arguments"
    return _err(ctx)


def _entry(fmt, name):
    return getattr(icx.lib(), f"icx_{fmt}_{name}")


class _Dev:
    """One file on the device, and the outputs of a batch of `n` slots of `stride` units."""

    def __init__(self, fmt, data, stride, n=1):
        import torch
        s = SPEC[fmt]
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.data = torch.from_numpy(np.frombuffer(data + bytes(16), np.uint8).copy()).to(self.dev)
        self.off = torch.zeros(n, dtype=torch.int64, device=self.dev)
        self.size = torch.full((n,), len(data), dtype=torch.int64, device=self.dev)
        self.out = torch.full((max(1, n * stride) * s["unit"] + 64,), 0xA5, dtype=torch.uint8, device=self.dev)
        self.status = torch.full((n,), -9, dtype=torch.int32, device=self.dev)
        self.dims = torch.full((n, s["ndims"]), -9, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize(self.dev)  # (the fills are done before another stream writes)

    def args(self, stride, out_shift=0, dims=True):
        return (self.data.data_ptr(), self.off.data_ptr(), self.size.data_ptr(), self.out.data_ptr() + out_shift, stride,
                self.status.data_ptr(), self.dims.data_ptr() if dims else None, None)

    def sync(self):
        self.torch.cuda.synchronize(self.dev)


# ------------------------------------------------------------------------------------ batch_create
@pytest.mark.parametrize("fmt", FMTS)
def test_create_refuses_each_limit_at_its_edge(ctx, fmt):
    s = SPEC[fmt]
    create, destroy = _entry(fmt, "batch_create"), _entry(fmt, "batch_destroy")
    for n, w, h in _COMMON_BAD + s["bad"]:
        _dirty(ctx)
        assert not create(ctx.ptr, n, w, h), (n, w, h)
        assert _err(ctx) == f"icx_{fmt}_batch_create: bad arguments", (n, w, h)
    for n, w, h in s["good"]:
        p = create(ctx.ptr, n, w, h)
        assert p, (n, w, h, _err(ctx))
        destroy(p)
    # without a context there is nothing to hold a message: null, and the create message unchanged
    before = icx.lib().icx_last_error(None)
    assert not create(None, 1, 1, 1)
    assert icx.lib().icx_last_error(None) == before


# ------------------------------------------------------------------------------------ batch_decode
@pytest.mark.parametrize("fmt", FMTS)
def test_decode_checks_in_order(ctx, fmt, files):
    s = SPEC[fmt]
    decode = _entry(fmt, "batch_decode")
    data = next(iter(files[fmt].values()))
    floor = s["floor"] * W * H_
    stride = max(floor, 64)
    b = s["cls"](ctx, 2, W, H_)
    try:
        d = _Dev(fmt, data, stride, 2)
        # nothing to do comes before any pointer check
        assert decode(b._p, 0, None, None, None, None, 0, None, None, None) == s["ok"]
        for n in (3, -1):
            _dirty(ctx)
            assert decode(b._p, n, *d.args(stride)) == s["internal"]
            assert _err(ctx) == f"icx_{fmt}_batch_decode: n exceeds batch capacity"
        # n is checked before the pointers, the pointers before the stride
        _dirty(ctx)
        assert decode(b._p, 3, None, None, None, None, 0, None, None, None) == s["internal"]
        assert _err(ctx) == f"icx_{fmt}_batch_decode: n exceeds batch capacity"
        _dirty(ctx)
        assert decode(b._p, 1, *d.args(0, dims=False)) == s["internal"]
        assert _err(ctx) == "null pointer"
        if floor:
            _dirty(ctx)
            assert decode(b._p, 1, *d.args(floor - 1)) == s["internal"]
            assert _err(ctx) == f"icx_{fmt}_batch_decode: out_stride too small"
            # (png: 59 is no multiple of 4 either; the floor is checked first)
        # the floor itself is accepted (pnm has none: a slot of 16 bytes holds the 15 of the P5 file)
        at = floor if floor else 16
        msg = _dirty(ctx)
        assert decode(b._p, 1, *d.args(at)) == s["ok"]
        d.sync()
        assert _err(ctx) == msg
        assert int(d.status.cpu()[0]) == s["ok"]
        assert [int(v) for v in d.dims.cpu()[0][:2]] == [W, H_]
    finally:
        b.close()


def test_png_refuses_unaligned_output(ctx, files):
    b = icx.PngBatch(ctx, 1, W, H_)
    try:
        stride = 4 * W * H_
        d = _Dev("png", files["png"]["rgb8"], stride)
        for shift, st in ((1, stride), (0, stride + 2)):
            _dirty(ctx)
            assert icx.lib().icx_png_batch_decode(b._p, 1, *d.args(st, shift)) == icx.PNGR_INTERNAL_ERR
            assert _err(ctx) == "icx_png_batch_decode: d_out and out_stride must be multiples of 4"
            with pytest.raises(icx.ICXError):
                b.decode_device(1, *d.args(st, shift))
    finally:
        b.close()


def test_pnm_returns_invalid_argument_for_unaligned_output(ctx, files):
    b = icx.PnmBatch(ctx, 1, W, H_)
    try:
        d = _Dev("pnm", files["pnm"]["p5"], 64)
        for shift, st in ((8, 64), (0, 72)):
            msg = _dirty(ctx)
            assert b.decode_device(1, *d.args(st, shift)) == icx.PNM_INVALID_ARGUMENT  # returned, not raised
            assert _err(ctx) == msg  # and no message
        assert b.decode_device(1, *d.args(64)) == icx.PNM_OK
        d.sync()
    finally:
        b.close()


# ------------------------------------------------------------------------------------ stage_times
@pytest.mark.parametrize("fmt", FMTS)
def test_stage_names_and_count(ctx, fmt):
    s = SPEC[fmt]
    b = s["cls"](ctx, 1, W, H_)
    try:
        assert list(b.stage_times()) == s["stages"]
        k = len(s["stages"])
        names, ms = (C.c_char_p * 8)(), (C.c_float * 8)(*([-1.0] * 8))
        times = _entry(fmt, "batch_stage_times")
        assert times(b._p, names, ms, 1) == k  # the full count, whatever the capacity
        assert names[0].decode() == s["stages"][0] and names[1] is None and ms[1] == -1.0
        assert times(b._p, None, None, 0) == k
        assert times(None, names, ms, 8) == 0
    finally:
        b.close()


# ------------------------------------------------------------------------------------ one-shot
def _one_shot(ctx, fmt, data):
    """-> (code, [the ints], array or None)"""
    got = getattr(ctx, fmt + "_decode")(data)
    return got[0], list(got[1:-1]), got[-1]


@pytest.mark.parametrize("fmt,variant", VARIANTS, ids=[f"{f}-{v}" for f, v in VARIANTS])
def test_one_shot_equals_batch_of_one(ctx, fmt, variant, files):
    s = SPEC[fmt]
    data = files[fmt][variant]
    code, ints, arr = _one_shot(ctx, fmt, data)
    assert code == s["ok"] and arr is not None
    assert ints[:2] == [W, H_] and arr.shape[:2] == (H_, W)
    stride = 4 * MW * MH
    b = s["cls"](ctx, 1, MW, MH)
    try:
        d = _Dev(fmt, data, stride)
        b.decode_device(1, *d.args(stride))
        d.sync()
    finally:
        b.close()
    dims = [int(v) for v in d.dims.cpu()[0]]
    assert int(d.status.cpu()[0]) == code
    assert dims[:len(ints)] == ints
    if len(ints) == 2:  # png, gif: the one-shot leaves the fixed depth out
        assert dims[2] == arr.shape[2]
    assert d.out.cpu().numpy()[:arr.nbytes].tobytes() == arr.tobytes()


@pytest.mark.parametrize("fmt", FMTS)
def test_one_shot_header_error(ctx, fmt):
    s = SPEC[fmt]
    data = b"\x07"
    pcode = s["probe"](data)[0]
    assert pcode not in (s["ok"], s["internal"])
    code, ints, arr = _one_shot(ctx, fmt, data)
    assert code == pcode and arr is None and ints == [0] * len(ints)
    # and through the C entry itself: a non-null `out` is nulled, the dims zeroed
    out = C.c_void_p(1)
    v = [C.c_int(-5) for _ in ints]
    buf = C.create_string_buffer(data, 1)
    assert _entry(fmt, "decode")(ctx.ptr, buf, 1, C.byref(out), *[C.byref(x) for x in v]) == pcode
    assert out.value is None and [x.value for x in v] == [0] * len(ints)


def test_hdr_one_shot_keeps_partial_image(ctx, files):
    """A file cut in the middle of its last row: not OK, yet the rows it had come back."""
    data = files["hdr"]["flat"]
    cut = data[:len(H.header(W, H_)) + 4 * W * (H_ - 1) + 6]
    code, w, h, rows, arr = ctx.hdr_decode(cut)
    assert code == icx.HDR_TRUNCATED and (w, h) == (W, H_)
    assert 0 < rows < H_ and arr is not None and arr.shape == (H_, W, 4)
    ref = O.hdr_decode(cut)
    assert (code, w, h, rows) == ref[:4]
    np.testing.assert_array_equal(arr.view(np.uint32), ref[4].view(np.uint32))
    full = ctx.hdr_decode(data)
    assert full[0] == icx.HDR_OK and full[3] == H_
    np.testing.assert_array_equal(arr[:rows].view(np.uint32), full[4][:rows].view(np.uint32))
