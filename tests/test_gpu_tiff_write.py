"""GPU TIFF write (Image::writeTiff; contract in include/icx.h "TIFF write") against the restatement
in tests/tiffwutil.py.

Compressions 1, 5 and 32773: the files equal the restatement's byte for byte. Deflate: every strip's
payload inflates (zlib, whole payload consumed) to the strip's differenced bytes, the file around the
payloads equals the restatement's, the tokens pass deflate_read.audit and no match crosses a 4096
multiple. Every file is at most icx_tiff_encode_bound, reads back through icx_tiff_decode (the batch
read, straight from the device slots the write filled) and through PIL to the pixels written.
Every batch has an odd out_stride, odd source addresses and sentinel bytes around each slot."""
import os
import zlib

import numpy as np
import pytest

import imagecodecs_amd as icx
import deflate_read as R
import tiffutil as T
import tiffwutil as W

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENT = 0xA5
PB_TILE = W.PB_TILE  # icx_tiffw.hip kPbTile


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def _a3(a):
    a = np.ascontiguousarray(a, np.uint8)
    return a[:, :, None] if a.ndim == 2 else a


def _encode(ctx, imgs, comp, pred, rps, stride=None, null=(), readback=True):
    """One icx_tiff_encode_device_batch -> (rc, status, sizes, files). Sources at odd addresses, an odd
    stride, sentinels before, between (a slot's bytes past its file) and after the slots. With
    readback, the batch read decodes the slots in place and the pixels must be the sources'."""
    import torch
    dev = torch.device("cuda", 0)
    imgs = [_a3(a) for a in imgs]
    n, d = len(imgs), imgs[0].shape[2]
    at, offs = 1, []
    for a in imgs:
        offs.append(at)
        at += a.size
        at += 1 - (at & 1)
    blob = np.zeros(at + 16, np.uint8)
    for a, o in zip(imgs, offs):
        blob[o:o + a.size] = a.reshape(-1)
    src = torch.from_numpy(blob).to(dev)
    bounds = [icx.tiff_encode_bound(a.shape[1], a.shape[0], d, comp, pred, rps) for a in imgs]
    if stride is None:
        stride = max(bounds + [8]) | 1
    out = torch.full((1 + n * stride + 64,), SENT, dtype=torch.uint8, device=dev)
    base = out.data_ptr() + 1
    assert base & 1 and all((src.data_ptr() + o) & 1 for o in offs) and stride & 1
    d_sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
    d_status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ptrs = [0 if i in null else src.data_ptr() + o for i, o in enumerate(offs)]
    rc = ctx.tiff_encode_device_batch(ptrs, [a.shape[1] for a in imgs], [a.shape[0] for a in imgs], d, comp, pred, rps,
                                      base, stride, d_sizes.data_ptr(), d_status.data_ptr())
    if rc != icx.TIFF_OK:
        return rc, None, None, None
    host = out.cpu().numpy()
    status, sizes = d_status.cpu().numpy(), d_sizes.cpu().numpy()
    files = []
    assert host[0] == SENT and (host[1 + n * stride:] == SENT).all(), "bytes outside the slots changed"
    for i in range(n):
        slot = host[1 + i * stride:1 + (i + 1) * stride]
        if status[i] == icx.TIFF_OK:
            assert 0 < sizes[i] <= bounds[i], (i, sizes[i], bounds[i])
            assert (slot[sizes[i]:] == SENT).all(), ("bytes after the file changed", i)
            files.append(slot[:sizes[i]].tobytes())
        else:
            assert (slot == SENT).all(), ("a failed image's slot changed", i, status[i])
            files.append(None)
    if readback and all(f is not None for f in files):
        mw, mh = max(a.shape[1] for a in imgs), max(a.shape[0] for a in imgs)
        tb = icx.TiffBatch(ctx, n, mw, mh)
        pstride = (4 * mw * mh + 15) & ~15
        pix = torch.zeros(n * pstride, dtype=torch.uint8, device=dev)
        st = torch.full((n,), -7, dtype=torch.int32, device=dev)
        dims = torch.zeros(3 * n, dtype=torch.int32, device=dev)
        foff = torch.tensor([1 + i * stride for i in range(n)], dtype=torch.int64, device=dev)
        tb.decode_device(n, out.data_ptr(), foff.data_ptr(), d_sizes.data_ptr(), pix.data_ptr(), pstride, st.data_ptr(),
                         dims.data_ptr())
        torch.cuda.synchronize()
        hp, hs, hd = pix.cpu().numpy(), st.cpu().numpy(), dims.cpu().numpy().reshape(n, 3)
        tb.close()
        for i, a in enumerate(imgs):
            assert hs[i] == icx.TIFF_OK and tuple(hd[i]) == (a.shape[1], a.shape[0], d), (i, hs[i], hd[i])
            np.testing.assert_array_equal(hp[i * pstride:i * pstride + a.size], a.reshape(-1), err_msg="read back %d" % i)
    return rc, status, sizes, files


def _check(files, imgs, comp, pred, rps, pil=True, name=""):
    """Files of compression 1 / 5 / 32773 equal the restatement's; Deflate files equal it around
    their own payloads, which zlib inflates, whole, to the strips' bytes."""
    for k, (f, a) in enumerate(zip(files, imgs)):
        a = _a3(a)
        what = (name, k, a.shape, comp, pred, rps)
        assert f is not None, what
        if comp != W.DEFLATE:
            assert f == W.write_tiff(a, comp, pred, rps), what
        else:
            H, pays = W.file_strips(f)
            r, n = W.geometry(a.shape[1], a.shape[0], a.shape[2], comp, pred, rps)
            raws = W.strips_raw(a, pred, r)
            assert len(pays) == n
            for p, raw in zip(pays, raws):
                z = zlib.decompressobj()
                assert z.decompress(p) == raw and z.eof and z.unused_data == b"", what
                assert p[:2] == b"\x78\x01"
            assert f == W.write_tiff(a, comp, pred, rps, payloads=pays), what
        if pil:
            np.testing.assert_array_equal(W.pil_pixels(f), a, err_msg="PIL " + str(what))


KINDS = ("noise", "smooth", "flat", "two_level")


def _make(kind, seed, h, w, d):
    if kind == "noise":
        return T.noise(seed, h, w, d).reshape(h, w, d)
    if kind == "smooth":
        return T.smooth(seed, h, w, d).reshape(h, w, d)
    if kind == "flat":
        return np.full((h, w, d), 40 + seed % 200, np.uint8)
    return (T.noise(seed, h, w, d, levels=2) * 199).astype(np.uint8).reshape(h, w, d)


def _grid(h):
    widths = list(range(1, 22)) + (list(range(253, 260)) + list(range(509, 516)) if h <= 3 else [])
    return widths


@pytest.mark.parametrize("d", (1, 3, 4))
@pytest.mark.parametrize("comp,pred", W.combos())
def test_files_over_the_grid(ctx, comp, pred, d):
    """d x compression x legal predictor x rps in {0, 1, 2, h-1, h, h+5}, widths 1..21 x heights 1..9
    and {253..259, 509..515} x 1..3, on noise, smooth, flat and two-level images (the kind rotates
    over the widths and the rps, so every width meets every kind)."""
    for h in range(1, 10):
        for j, rps in enumerate(W.rps_set(h)):
            imgs = [_make(KINDS[(w + j) % 4], w * 16 + h, h, w, d) for w in _grid(h)]
            rc, status, sizes, files = _encode(ctx, imgs, comp, pred, rps)
            assert rc == icx.TIFF_OK and (status == icx.TIFF_OK).all(), (h, rps, status)
            _check(files, imgs, comp, pred, rps, name="grid")


def test_lzw_edges(ctx):
    """The a, b sequence (one code per byte) cut so that the strip's end and the EOI fall on each
    width step and on both sides of the forced Clear; 65,280 bytes in one strip (17 Clears); two-level
    noise of 64 KiB (long strings, a full table); an all-equal 64 KiB strip (strings of 1, 2, 3 ...)."""
    cases = W.lzw_edge_images()
    imgs = [a for _, a in cases]
    rc, status, sizes, files = _encode(ctx, imgs, W.LZW, 1, 0)
    assert rc == icx.TIFF_OK and (status == icx.TIFF_OK).all(), status
    for (name, a), f in zip(cases, files):
        _check([f], [a], W.LZW, 1, 0, name=name)
    # the same bytes as strips of a larger image, differenced
    big = [a for n, a in cases if n in ("ab_all", "two_level")]
    rc, status, sizes, files = _encode(ctx, big, W.LZW, 2, 15)
    assert rc == icx.TIFF_OK and (status == icx.TIFF_OK).all()
    _check(files, big, W.LZW, 2, 15, name="lzw strips")


def test_packbits_edges(ctx):
    """Runs of 1, 2, 3, 127 .. 131, 256 .. 258 at a row's start, middle and end; the same byte over a
    row end (cut there); literal stretches of 127, 128, 129, 257; a 2-run between literals; rows of 1
    and 2 bytes; rows of 16 tiles less 24 bytes and more, PB_TILE (the kernel's kPbTile, read from its
    source) being the positions a wave takes per step."""
    cases = W.packbits_edge_images()
    assert max(a.shape[1] for _, a in cases) > 8 * PB_TILE and dict(cases)["long_row_one_run"].shape[1] % PB_TILE
    imgs = [a for _, a in cases]
    for rps in (0, 1, 2):
        rc, status, sizes, files = _encode(ctx, imgs, W.PACKBITS, 1, rps)
        assert rc == icx.TIFF_OK and (status == icx.TIFF_OK).all(), status
        for (name, a), f in zip(cases, files):
            _check([f], [a], W.PACKBITS, 1, rps, name=name)


def test_deflate_strip_sizes_and_audit(ctx):
    """One-row grey strips of 4095, 4096, 4097, 65535, 65536, 65537 and 2 x 65536 bytes straddle the
    segment (4096) and block (16 segments) limits; smooth and flat files pass the token audit
    (properties (a) to (f) of deflate_read.audit) and no match crosses a 4096 multiple; noise stays
    under the bound (_encode asserts size <= bound for every file)."""
    sizes_ = (4095, 4096, 4097, 65535, 65536, 65537, 2 * 65536)
    for kind in ("smooth", "flat", "noise"):
        imgs = [_make(kind, n, 1, n, 1) for n in sizes_]
        for pred in (1, 2):
            rc, status, sizes, files = _encode(ctx, imgs, W.DEFLATE, pred, 0)
            assert rc == icx.TIFF_OK and (status == icx.TIFF_OK).all(), (kind, status)
            _check(files, imgs, W.DEFLATE, pred, 0, name=kind)
            for f, a in zip(files, imgs):
                H, pays = W.file_strips(f)
                raw = W.strips_raw(a, pred, a.shape[0])[0]
                blocks = R.read_zlib(pays[0])
                assert len(blocks) == -(-len(raw) // 65536), (len(raw), len(blocks))
                assert R.crossing(blocks, 4096) == [], ("a match crosses a segment end", kind, len(raw))
                if kind != "noise":
                    R.audit(blocks, raw, log=print)
    # rows above: a smooth RGB image in strips of several rows
    a = _make("smooth", 3, 40, 300, 3)
    rc, status, sizes, files = _encode(ctx, [a], W.DEFLATE, 2, 16)
    assert (status == icx.TIFF_OK).all()
    _check(files, [a], W.DEFLATE, 2, 16)
    for p, raw in zip(W.file_strips(files[0])[1], W.strips_raw(a, 2, 16)):
        blocks = R.read_zlib(p)
        R.audit(blocks, raw, log=print)
        assert R.crossing(blocks, 4096) == []


def test_deflate_all_equal_strip_is_small(ctx):
    """An all-equal 64 KiB strip compresses to under 1/50 of its size (the EXR writer's figure for the
    same back end is 334 bytes of 160,000: this only catches a dead matcher)."""
    a = np.full((256, 256), 77, np.uint8)
    rc, status, sizes, files = _encode(ctx, [a], W.DEFLATE, 1, 0)
    assert (status == icx.TIFF_OK).all()
    _check(files, [a], W.DEFLATE, 1, 0)
    pay = W.file_strips(files[0])[1][0]
    print("all-equal 65536-byte strip ->", len(pay), "bytes")
    assert len(pay) * 50 < 65536, len(pay)


@pytest.mark.parametrize("comp,pred", W.combos())
def test_fixture_pixels_round_trip(ctx, comp, pred):
    """The pixels of the reference's test.tif, written under each compression in 64-row strips and
    as one strip, read back to themselves (save_to_memory -> tiff_decode, and PIL)."""
    src = open(os.path.join(GOLDEN, "tiff", "test.tif"), "rb").read()
    code, w, h, d, px = ctx.tiff_decode(src)
    assert (code, w, h, d) == (icx.TIFF_OK, 499, 289, 3)
    for rps in (64, 0):
        code, f = ctx.tiff_save_to_memory(px, comp, pred, rps)
        assert code == icx.TIFF_OK and len(f) <= icx.tiff_encode_bound(w, h, d, comp, pred, rps)
        _check([f], [px], comp, pred, rps, name="fixture")
        back = ctx.tiff_decode(f)
        assert back[:4] == (icx.TIFF_OK, w, h, d)
        np.testing.assert_array_equal(back[4], px)


@pytest.mark.parametrize("d", (1, 3, 4))
def test_host_entry_round_trip(ctx, d):
    """icx_tiff_decode(icx_tiff_save_to_memory(x)) == x through the host entries (one image up, one file
    back, the bound as the slot), for every compression x legal predictor x rps in {0, 1, 2, h-1, h, h+5}
    at a few odd sizes; the files are the restatement's (Deflate: around their own payloads)."""
    for comp, pred in W.combos():
        for k, (w, h) in enumerate(((1, 1), (21, 9), (7, 5), (259, 3), (513, 2))):
            for j, rps in enumerate(W.rps_set(h)):
                a = _make(KINDS[(k + j) % 4], w + h + d, h, w, d)
                code, f = ctx.tiff_save_to_memory(a, comp, pred, rps)
                assert code == icx.TIFF_OK and len(f) <= icx.tiff_encode_bound(w, h, d, comp, pred, rps), (comp, pred, w, h, rps)
                _check([f], [a], comp, pred, rps, pil=False, name="host entry")
                back = ctx.tiff_decode(f)
                assert back[:4] == (icx.TIFF_OK, w, h, d), (back[:4], comp, pred, w, h, rps)
                np.testing.assert_array_equal(back[4], a)


def test_statuses(ctx):
    a = _make("smooth", 1, 9, 21, 3)
    # call-level refusals
    for args in ((7, 1, 0), (1, 2, 0), (32773, 2, 0), (5, 3, 0), (8, 0, 0), (1, 1, -1)):
        assert _encode(ctx, [a], *args)[0] == icx.TIFF_INVALID_ARGUMENT, args
    assert _encode(ctx, [a[:, :, :2]], 1, 1, 0)[0] == icx.TIFF_INVALID_ARGUMENT  # d = 2
    L = icx.lib()
    assert L.icx_tiff_encode_device_batch(ctx.ptr, -1, None, None, None, 3, 1, 1, 0, None, 0, None, None, None) == icx.TIFF_INVALID_ARGUMENT
    assert L.icx_tiff_encode_device_batch(ctx.ptr, 65536, None, None, None, 3, 1, 1, 0, None, 0, None, None, None) == icx.TIFF_INVALID_ARGUMENT
    assert L.icx_tiff_encode_device_batch(ctx.ptr, 1, None, None, None, 3, 1, 1, 0, None, 0, None, None, None) == icx.TIFF_INVALID_ARGUMENT
    assert L.icx_tiff_encode_device_batch(ctx.ptr, 0, None, None, None, 3, 1, 1, 0, None, 0, None, None, None) == icx.TIFF_OK  # n = 0
    # save_to_memory's refusals
    assert ctx.tiff_save_to_memory(a, 8, 3, 0) == (icx.TIFF_INVALID_ARGUMENT, None)
    assert ctx.tiff_save_to_memory(a, 32773, 2, 0) == (icx.TIFF_INVALID_ARGUMENT, None)
    assert ctx.tiff_save_to_memory(a.astype(np.uint16), 1, 1, 0) == (icx.TIFF_INVALID_ARGUMENT, None)
    assert ctx.tiff_save_to_memory(np.zeros((0, 4, 3), np.uint8), 1, 1, 0) == (icx.TIFF_INVALID_ARGUMENT, None)
    # per-image refusals by size, in a batch beside a good image: more than 2^30 pixels, a strip of 2^31
    # bytes, a worst-case file of 2^32 bytes (the sources are never read: the first image's stand in)
    import torch
    dev = torch.device("cuda", 0)
    for d_, ws, hs, rps in ((1, [32769, 21], [32768, 9], 1 << 20), (4, [1 << 29, 21], [2, 9], 1), (4, [1 << 15, 21], [1 << 15, 9], 8)):
        stride = icx.tiff_encode_bound(21, 9, d_, 1, 1, rps) | 1
        good = _make("noise", 6, 9, 21, d_)
        src_ = torch.from_numpy(good.reshape(-1)).to(dev)
        out = torch.full((2 * stride,), SENT, dtype=torch.uint8, device=dev)
        d_sizes = torch.full((2,), -1, dtype=torch.int64, device=dev)
        d_status = torch.full((2,), -7, dtype=torch.int32, device=dev)
        assert icx.tiff_encode_bound(ws[0], hs[0], d_, 1, 1, rps) == 0
        rc = ctx.tiff_encode_device_batch([src_.data_ptr()] * 2, ws, hs, d_, 1, 1, rps, out.data_ptr(), stride, d_sizes.data_ptr(),
                                          d_status.data_ptr())
        assert rc == icx.TIFF_OK and list(d_status.cpu().numpy()) == [icx.TIFF_INVALID_ARGUMENT, icx.TIFF_OK], (ws, hs)
        host = out.cpu().numpy()
        assert int(d_sizes[0]) == 0 and (host[:stride] == SENT).all()
        assert host[stride:stride + int(d_sizes[1])].tobytes() == W.write_tiff(good, 1, 1, rps)
    # TOO_LARGE at size - 1 (nothing written, the size reported), success at size
    for comp, pred in W.combos():
        rc, status, sizes, files = _encode(ctx, [a], comp, pred, 4)
        size = int(sizes[0])
        assert size & 1 == 0
        rc, status, sizes, files = _encode(ctx, [a], comp, pred, 4, stride=size - 1)
        assert rc == icx.TIFF_OK and status[0] == icx.TIFF_TOO_LARGE and sizes[0] == size and files[0] is None
        rc, status, sizes, files = _encode(ctx, [a], comp, pred, 4, stride=size + 1)  # (an odd stride again)
        assert status[0] == icx.TIFF_OK and sizes[0] == size
    # a mixed batch: valid, null source, bad size, too large (a larger image with the first's stride)
    small, large = _make("noise", 2, 4, 5, 3), _make("noise", 3, 30, 40, 3)
    zero = np.zeros((4, 5, 3), np.uint8)
    for comp, pred in W.combos():
        stride = icx.tiff_encode_bound(5, 4, 3, comp, pred, 2) | 1
        imgs = [small, zero, small, large]
        dev = torch.device("cuda", 0)
        srcs = [torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dev) for x in imgs]
        out = torch.full((4 * stride + 8,), SENT, dtype=torch.uint8, device=dev)
        d_sizes = torch.full((4,), -1, dtype=torch.int64, device=dev)
        d_status = torch.full((4,), -7, dtype=torch.int32, device=dev)
        rc = ctx.tiff_encode_device_batch([srcs[0].data_ptr(), 0, srcs[2].data_ptr(), srcs[3].data_ptr()], [5, 5, 0, 40],
                                          [4, 4, 4, 30], 3, comp, pred, 2, out.data_ptr(), stride, d_sizes.data_ptr(),
                                          d_status.data_ptr())
        assert rc == icx.TIFF_OK
        st, sz, host = d_status.cpu().numpy(), d_sizes.cpu().numpy(), out.cpu().numpy()
        assert list(st) == [icx.TIFF_OK, icx.TIFF_INVALID_ARGUMENT, icx.TIFF_INVALID_ARGUMENT, icx.TIFF_TOO_LARGE], (comp, st)
        assert sz[1] == 0 and sz[2] == 0 and sz[3] > stride and (host[stride:] == SENT).all()
        _check([host[:sz[0]].tobytes()], [small], comp, pred, 2, name="mixed")
        assert (host[sz[0]:stride] == SENT).all()
    # 4096 strips accepted, 4097 refused (as an image of the batch, and by the bound)
    tall = _make("noise", 4, 4097, 1, 1)
    rc, status, sizes, files = _encode(ctx, [tall[:4096]], W.LZW, 1, 1)
    assert status[0] == icx.TIFF_OK
    _check(files, [tall[:4096]], W.LZW, 1, 1, pil=False, name="4096 strips")
    rc, status, sizes, files = _encode(ctx, [tall, tall[:5]], W.LZW, 1, 1, stride=8191)
    assert rc == icx.TIFF_OK and list(status) == [icx.TIFF_INVALID_ARGUMENT, icx.TIFF_OK] and sizes[0] == 0
    assert icx.tiff_encode_bound(1, 4097, 1, 5, 1, 1) == 0 and icx.tiff_encode_bound(1, 4096, 1, 5, 1, 1) > 0


def test_python_image_write_tiff(ctx, tmp_path, capsys):
    """Image.writeTiff, defaults and explicit arguments, gives save_to_memory's bytes (which are
    icx_tiff_save_to_file's: tests/test_cxx_tiff_write.py); another type writes nothing; write(".tif")
    still raises."""
    a = _make("smooth", 5, 11, 23, 3)
    img = icx.Image()
    img.load(a.reshape(-1), 23, 11, 3)
    p = str(tmp_path / "named.anything")
    img.writeTiff(p)
    assert open(p, "rb").read() == ctx.tiff_save_to_memory(a, 8, 1, 0)[1]
    img.writeTiff(p, icx.TIFF_COMPRESSION_LZW, 2, 3)
    assert open(p, "rb").read() == ctx.tiff_save_to_memory(a, 5, 2, 3)[1] == W.write_tiff(a, 5, 2, 3)
    q = str(tmp_path / "u16.tif")
    u = icx.Image()
    u.load(np.zeros(16, np.uint16), 4, 4, 1, icx.Image.USHORT)
    u.writeTiff(q)
    assert not os.path.exists(q) and "only UBYTE" in capsys.readouterr().err
    img.writeTiff(q, 32773, 2, 0)  # a refused combination: a line, no file
    assert not os.path.exists(q)
    with pytest.raises(ValueError):
        img.write(str(tmp_path / "x.tif"))
