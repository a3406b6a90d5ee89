"""GPU BMP read and write (Image::readBmp / writeBmp, codecs.cpp:255-375; contract in include/icx.h)
against the restatement in tests/bmputil.py and the reference's data/test.bmp.

Read: status, size, channels and every output byte of every file of the shared case lists equal the
restatement's. Write: the bytes equal the restatement's, decode(encode(x)) == x, and writing the
fixture's pixels reproduces the fixture's raster."""
import hashlib
import io
import os
import struct

import numpy as np
import pytest

import imagecodecs_amd as icx
import bmputil as B

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = open(os.path.join(GOLDEN, "bmp", "test.bmp"), "rb").read()
KBMP_TILE = 4096  # icx_bmp.hip kBmpTile: stream bytes per tile of k_bmp_tiles / k_bmp_expand
KBMP_SEG = 1024   # kBmpSeg: pixels per row segment of the streaming kernels
STAGES = {"parse", "locate", "fill", "expand", "raw"}


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fixture_px():
    return B.decode(FIXTURE)[4]


def _same(got, data, name=""):
    ref = B.decode(data)
    assert got[0] == ref[0], (name, got[0], ref[0])
    if ref[0] == B.OK:
        assert got[1:4] == ref[1:4], name
        np.testing.assert_array_equal(got[4], ref[4], err_msg=name)
    else:
        assert got[1:4] == (0, 0, 0) and got[4] is None, name


def _batch(ctx, files, max_w, max_h, pad=0):
    """One icx_bmp_batch_decode over `files` -> per-image (code, w, h, d, pixels or None), stage times.
    Guard bytes before, after and behind each image's pixels must come back untouched."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(files)
    sizes = np.array([len(f) for f in files], np.int64)
    offs = np.zeros(n, np.int64)
    offs[1:] = np.cumsum(sizes)[:-1]
    blob = b"".join(files) or b"\0"
    data = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(offs).to(dev)
    d_sz = torch.from_numpy(sizes).to(dev)
    stride = 4 * max_w * max_h + pad
    guard = 256
    out = torch.full((guard + n * stride + guard,), 0xA5, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    dims = torch.full((n, 3), -9, dtype=torch.int32, device=dev)
    b = icx.BmpBatch(ctx, n, max_w, max_h)
    stream = torch.cuda.current_stream(dev).cuda_stream
    torch.cuda.synchronize(dev)  # (the fills above are done before another stream writes)
    b.decode_device(n, data.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), out.data_ptr() + guard, stride,
                    st.data_ptr(), dims.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    times = b.stage_times()
    b.close()
    out, st, dims = out.cpu().numpy(), st.cpu().numpy(), dims.cpu().numpy()
    assert (out[:guard] == 0xA5).all() and (out[-guard:] == 0xA5).all()
    res = []
    for i in range(n):
        w, h, d = (int(v) for v in dims[i])
        slot = out[guard + i * stride: guard + (i + 1) * stride]
        arr = None
        if st[i] == icx.BMP_OK:
            arr = slot[:w * h * d].reshape(h, w, d)
            assert (slot[w * h * d:] == 0xA5).all(), f"image {i} wrote past its pixels"
        res.append((int(st[i]), w, h, d, arr))
    return res, times


def _check_batch(ctx, cases, max_w, max_h, pad=0):
    res, times = _batch(ctx, [f for _, f in cases], max_w, max_h, pad)
    for (name, f), got in zip(cases, res):
        _same(got, f, name)
    return times


# ------------------------------------------------------------------------------------ read
def test_bmp_fixture(ctx, fixture_px):
    got = ctx.bmp_decode(FIXTURE)
    assert got[:4] == (icx.BMP_OK, 499, 289, 3)
    assert hashlib.sha256(got[4].tobytes()).hexdigest() == B.FIXTURE_SHA256
    np.testing.assert_array_equal(got[4], fixture_px)


def test_bmp_raw_depths_widths_heights(ctx):
    """Every raw depth x widths 1-9, 31-33, 127-129, 395, 499 x heights 1, 2, 3, 17, both row orders."""
    cases = B.raw_cases()
    assert len(cases) == 6 * 17 * 4 * 2
    assert set(_check_batch(ctx, cases, 499, 17)) == STAGES


def test_bmp_raw_single_decode(ctx):
    """The one-image entry (a workspace without tile tables) on one file of each depth and order."""
    for name, f in B.raw_cases():
        if "_129x3_" in name or "_499x17_" in name:
            _same(ctx.bmp_decode(f), f, name)


def test_bmp_offbits_headers_palettes_masks(ctx):
    cases = B.offbits_cases() + B.header_cases() + B.palette_cases() + B.mask_cases()
    names = {n for n, _ in cases}
    assert {f"off24_{g}" for g in range(16)} <= names and {f"hs{h}_24" for h in B.HEADER_SIZES} <= names
    _check_batch(ctx, cases, 130, 3)
    by = dict(cases)
    for name, d in (("grey256", 1), ("grey255", 1), ("grey_core", 1), ("grey_one_off", 3), ("mask_4444_alpha_5", 4),
                    ("mask_5551_5", 4), ("mask_zero_alpha_5", 3), ("mask_101010_5", 3), ("hs108_fields32", 4), ("hs52_fields32", 3)):
        got = ctx.bmp_decode(by[name])
        assert got[3] == d, name
        _same(got, by[name], name)


def test_bmp_wide_raw_rows(ctx):
    """Rows longer than one segment of the streaming kernel (1024 pixels), every depth."""
    cases = [(f"wide{bits}", B.raw_file(60 + bits, bits, 1024 + 37 * k + 1, 3, topdown=bool(k & 1), gap=k))
             for k, bits in enumerate(B.DEPTHS)]
    cases.append(("wide_alpha", B.raw_file(70, 32, 2050, 2, comp=6, masks=B.M8888)))
    _check_batch(ctx, cases, 2100, 3, 5)


@pytest.mark.parametrize("rle", [8, 4])
def test_bmp_rle_shapes(ctx, rle):
    cases = B.rle_shape_cases(rle)
    names = {n[len(f"rle{rle}_"):] for n, _ in cases}
    assert {"run1", "run2", "run254", "run255", "lit3", "lit4", "lit5", "lit255", "run255_clipped", "lit255_clipped",
            "eol_mid_row", "delta_0_0", "delta_255_255", "delta_1_255", "y_past_h", "early_eob", "no_eob", "nibble_phase"} <= names
    for name, f in cases:
        assert B.decode(f)[0] == B.OK, name
        _same(ctx.bmp_decode(f), f, name)
    _check_batch(ctx, cases, 300, 300)


@pytest.mark.parametrize("rle", [8, 4])
def test_bmp_stream_over_three_tiles(ctx, rle):
    f = B.tiled_case(rle, KBMP_TILE)
    off, = struct.unpack_from("<I", f, 10)
    assert len(f) - off > 3 * KBMP_TILE
    _same(ctx.bmp_decode(f), f, "tiled")
    cut = f[:off + 2 * KBMP_TILE + 1]  # the stream ends one byte into the third tile
    _same(ctx.bmp_decode(cut), cut, "tiled_cut")
    _check_batch(ctx, [("tiled", f), ("tiled_cut", cut), ("tiled_again", f)], 211, 400, 1)


@pytest.mark.parametrize("rle", [8, 4])
def test_bmp_packets_across_tile_edges(ctx, rle):
    """A 4-byte delta packet and a 255-pixel absolute packet at every even offset across the first
    two tile edges: each later tile's entry slot and cursor come from the tile before it."""
    cases = B.edge_cases(rle, KBMP_TILE)
    assert len(cases) == 2 * (3 + (130 if rle == 8 else 66))
    _check_batch(ctx, cases, 300, 80)
    name, f = cases[len(cases) // 2]
    _same(ctx.bmp_decode(f), f, name)


# ------------------------------------------------------------------------------------ errors, batches
def test_bmp_every_status(ctx):
    cases = B.error_cases()
    for name, f, code in cases:
        got = ctx.bmp_decode(f)
        assert got[0] == code, name
        _same(got, f, name)
    small = [(n, f) for n, f, c in cases if c != B.TOO_LARGE]
    _check_batch(ctx, small, 16, 8, 3)


def test_bmp_prefixes_and_bit_flips(ctx):
    """Every prefix and 200 seeded bit flips of one 24-bit and one RLE8 file."""
    for k, src in enumerate(B.fuzz_sources()):
        _check_batch(ctx, [(f"prefix{k}_{len(p)}", p) for p in B.prefixes(src)], 16, 8)
        flips = [(f"flip{k}_{j}", p) for j, p in enumerate(B.bit_flips(src, 77 + k))]
        assert len(flips) == 200
        _check_batch(ctx, flips, 255, 255)


def test_bmp_batch_mixed(ctx):
    """Failed images between good ones, raw and run-length coded, in one call."""
    good = [B.raw_cases()[k] for k in (0, 100, 333, 500, 700, 815)] + B.rle_shape_cases(8)[:6] + B.rle_shape_cases(4)[-6:]
    bad = [(n, f) for n, f, c in B.error_cases() if c not in (B.OK, B.TOO_LARGE)]
    cases = []
    for k, g in enumerate(good):
        cases += [g, bad[(3 * k) % len(bad)], bad[(3 * k + 1) % len(bad)]]
    cases = [(n, f) for n, f in cases if B.decode(f)[0] != B.OK or (B.decode(f)[1] <= 300 and B.decode(f)[2] <= 20)]
    assert sum(B.decode(f)[0] == B.OK for _, f in cases) >= 10
    assert set(_check_batch(ctx, cases, 300, 20)) == STAGES


@pytest.mark.parametrize("pad", [1, 2, 3])
def test_bmp_batch_unaligned_stride(ctx, pad):
    """out_stride not a multiple of 16: images 1.. start off 16-byte alignment, so the ragged ends
    of the streaming, fill and expand kernels are what write them."""
    cases = [(f"u{bits}", B.raw_file(80 + bits, bits, 61 + k, 7, topdown=bool(k & 1), gap=k)) for k, bits in enumerate(B.DEPTHS)]
    cases.append(("u_alpha", B.raw_file(90, 16, 70, 7, comp=6, masks=B.M4444)))
    cases.append(("u_grey", B.raw_file(91, 8, 70, 7, palette=B.grey_palette())))
    cases += [(f"u_rle{rle}", B.rle_file(rle, 70, 7, B.random_stream(5 + rle, rle, 600, 70) + B.EOB)) for rle in (8, 4)]
    cases.append(("u_rle_grey", B.rle_file(8, 70, 7, B.random_stream(3, 8, 300, 70), palette=B.grey_palette())))
    _check_batch(ctx, cases, 70, 7, pad)


def test_bmp_too_large_for_workspace(ctx):
    wide = B.raw_file(1, 24, 33, 4)
    tall = B.rle_file(8, 8, 21, B.run(3, 1) + B.EOB)
    ok = B.raw_file(2, 4, 32, 20)
    okr = B.rle_file(4, 32, 20, B.random_stream(9, 4, 500, 32) + B.EOB)
    # a stream longer than the workspace covers (2*32*20 + 2*20 + 2 bytes) whose walk has not ended by then
    long_stream = B.rle_file(8, 32, 20, B.delta(0, 0) * 1200 + B.run(3, 1) + B.EOB)
    # and one as long whose walk ends inside the part the workspace covers
    long_tail = B.rle_file(8, 32, 20, B.run(3, 1) + B.EOB + bytes(5000))
    res, _ = _batch(ctx, [wide, ok, tall, okr, long_stream, long_tail], 32, 20)
    for k in (0, 2, 4):
        assert res[k][:4] == (icx.BMP_TOO_LARGE, 0, 0, 0), k
    _same(res[1], ok)
    _same(res[3], okr)
    _same(res[5], long_tail)
    _same(ctx.bmp_decode(long_stream), long_stream)  # (the one-image entry sizes its workspace by the file)


# ------------------------------------------------------------------------------------ write
@pytest.mark.parametrize("d", [1, 3, 4])
def test_bmp_encode_bytes(ctx, d):
    for w in (1, 2, 3, 4, 5, 6, 7, 8, 9, 499):
        px = B.synth(400 + w + d, w, 4, d)
        code, data = ctx.bmp_save_to_memory(px)
        assert code == icx.BMP_OK and data == B.encode(px), (w, d)
        assert len(data) == icx.bmp_encode_bound(w, 4, d)
        ref = B.decode(data)
        assert ref[:4] == (B.OK, w, 4, d) and (ref[4] == px).all()
        got = ctx.bmp_decode(data)
        assert got[:4] == (icx.BMP_OK, w, 4, d) and (got[4] == px).all()


def test_bmp_encode_wide_rows(ctx):
    for d in (1, 3, 4):
        px = B.synth(7 + d, 1024 + 13 * d, 3, d)
        code, data = ctx.bmp_save_to_memory(px)
        assert code == icx.BMP_OK and data == B.encode(px), d


def test_bmp_encode_reproduces_the_fixture(ctx, fixture_px):
    code, data = ctx.bmp_save_to_memory(fixture_px)
    assert code == icx.BMP_OK and len(data) == len(FIXTURE) and data[54:] == FIXTURE[54:]
    for at, fmt in ((18, "<i"), (22, "<i"), (28, "<H"), (34, "<I")):  # biWidth, biHeight, biBitCount, biSizeImage
        assert struct.unpack_from(fmt, data, at) == struct.unpack_from(fmt, FIXTURE, at), at


def test_bmp_written_files_open_in_pil(ctx):
    from PIL import Image  # (no skip: PIL reading the written files is part of what is checked)
    for d in (1, 3, 4):
        for w in (1, 2, 3, 4, 5, 6, 7, 8, 9, 499):
            px = B.synth(20 * d + w, w, 3, d)
            code, data = ctx.bmp_save_to_memory(px)
            assert code == icx.BMP_OK
            im = Image.open(io.BytesIO(data))
            assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[d]
            assert (np.asarray(im).reshape(px.shape) == px).all(), (d, w)


def test_bmp_encode_bad_arguments(ctx):
    for shape in ((4, 4, 2), (4, 4, 5), (0, 4, 3), (4, 0, 3), (65536, 1, 1), (1, 65536, 1), (2, 2, 2, 2)):
        assert ctx.bmp_save_to_memory(np.zeros(shape, np.uint8)) == (icx.BMP_INVALID_ARGUMENT, None), shape
    assert ctx.bmp_encode_device_batch([1], [4], [4], 2, 1, 100, 1, 1) == icx.BMP_INVALID_ARGUMENT
    assert ctx.bmp_encode_device_batch([1], [4], [4], 3, 0, 100, 1, 1) == icx.BMP_INVALID_ARGUMENT


@pytest.mark.parametrize("d", [1, 3, 4])
def test_bmp_encode_device_batch(ctx, d):
    """Three images in one call at an odd out_stride, a fourth with a bad width and a fifth whose
    file does not fit: each gets its own status, the neighbours' files are intact."""
    import torch
    dev = torch.device("cuda", 0)
    imgs = [B.synth(80 + k, w, h, d) for k, (w, h) in enumerate([(129, 7), (40, 33), (257, 5)])]
    big = B.synth(1, 90, 70, d)
    srcs = [torch.from_numpy(p.copy()).to(dev) for p in imgs + [imgs[0], big]]
    widths = [p.shape[1] for p in imgs] + [0, 90]
    heights = [p.shape[0] for p in imgs] + [7, 70]
    stride = max(B.encode_bound(p.shape[1], p.shape[0], d) for p in imgs) + 3
    stride += 1 - stride % 2
    assert stride % 2 == 1 and stride < B.encode_bound(90, 70, d)
    n = len(srcs)
    out = torch.full((n * stride + 64,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = torch.zeros((n,), dtype=torch.int64, device=dev)
    status = torch.full((n,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)  # (the fills above are done before the context's stream writes)
    rc = ctx.bmp_encode_device_batch([s.data_ptr() for s in srcs], widths, heights, d, out.data_ptr(), stride,
                                     sizes.data_ptr(), status.data_ptr())
    assert rc == icx.BMP_OK
    out, sizes, status = out.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy()
    assert list(status) == [icx.BMP_OK] * 3 + [icx.BMP_INVALID_ARGUMENT, icx.BMP_TOO_LARGE]
    assert sizes[3] == 0 and sizes[4] == B.encode_bound(90, 70, d)
    for i, px in enumerate(imgs):
        want = B.encode(px)
        slot = out[i * stride:(i + 1) * stride]
        assert sizes[i] == len(want) and slot[:len(want)].tobytes() == want, i
        assert (slot[len(want):] == 0xA5).all(), i
    assert (out[3 * stride:] == 0xA5).all()


@pytest.mark.parametrize("pad", [1, 2, 3])
def test_bmp_segment_edges_write_and_read(ctx, pad):
    """1 x 1, 5 x 2 and (KBMP_SEG + 1) x 2, every channel count, the pixels at an odd device address
    and the files' stride padded by 1, 2 or 3 bytes: file rows shorter than 16 bytes that start off
    alignment, a ragged head before the 16-byte stores and a tail after them, a second row segment
    of one pixel, and window loads whose first and last 16 bytes straddle the source's ends. The
    files are then read back in one batch behind an odd number of bytes, slots padded the same."""
    import torch
    dev = torch.device("cuda", 0)
    shapes = ((1, 1), (5, 2), (KBMP_SEG + 1, 2))
    off = 2 * pad + 1
    cases = [("odd", b"\xEE" * off)]  # (not a BMP: it only moves the files after it)
    for d in (1, 3, 4):
        imgs = [B.synth(30 * d + w, w, h, d) for w, h in shapes]
        bufs = [torch.from_numpy(np.frombuffer(bytes(off) + p.tobytes(), np.uint8).copy()).to(dev) for p in imgs]
        stride = B.encode_bound(KBMP_SEG + 1, 2, d) + pad
        n = len(imgs)
        out = torch.full((n * stride + 64,), 0xA5, dtype=torch.uint8, device=dev)
        sizes = torch.zeros((n,), dtype=torch.int64, device=dev)
        status = torch.full((n,), -9, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)  # (the fills above are done before the context's stream writes)
        rc = ctx.bmp_encode_device_batch([b.data_ptr() + off for b in bufs], [w for w, _ in shapes], [h for _, h in shapes], d,
                                         out.data_ptr(), stride, sizes.data_ptr(), status.data_ptr())
        assert rc == icx.BMP_OK and list(status.cpu().numpy()) == [icx.BMP_OK] * n
        o = out.cpu().numpy()
        for i, px in enumerate(imgs):
            want = B.encode(px)
            slot = o[i * stride:(i + 1) * stride]
            assert slot[:len(want)].tobytes() == want and (slot[len(want):] == 0xA5).all(), (d, i)
            cases.append((f"d{d}_{px.shape[1]}x{px.shape[0]}", want))
        assert (o[n * stride:] == 0xA5).all()
    _check_batch(ctx, cases, KBMP_SEG + 1, 2, pad)


# ------------------------------------------------------------------------------------ icx.Image
def test_image_read_bmp(tmp_path, fixture_px):
    p = tmp_path / "x.BMP"
    p.write_bytes(FIXTURE)
    img = icx.Image()
    img.read(str(p))
    assert (img.cols(), img.rows(), img.channels(), img.type()) == (499, 289, 3, icx.Image.UBYTE)
    assert img.totalBytes() == 499 * 289 * 3 and img.data().tobytes() == fixture_px.tobytes()
    none = tmp_path / "none.bmp"
    none.write_bytes(b"BN" + FIXTURE[2:200])
    with pytest.raises(RuntimeError):
        icx.Image().read(str(none))


@pytest.mark.parametrize("d", [1, 3, 4])
def test_image_write_read_round_trip(tmp_path, d):
    px = B.synth(90 + d, 67, 31, d)
    img = icx.Image()
    img.load(px, 67, 31, d)
    p = tmp_path / f"rt{d}.bmp"
    img.write(str(p))
    assert p.read_bytes() == B.encode(px)
    back = icx.Image()
    back.read(str(p))
    assert (back.cols(), back.rows(), back.channels()) == (67, 31, d)
    assert back.data().tobytes() == px.tobytes()
