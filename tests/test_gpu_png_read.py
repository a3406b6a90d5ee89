"""GPU PNG read (icx_png_decode / icx_png_batch_* / Image.read(".png")): bit-exact against
tests/pngutil.decode_rgba (zlib + numpy, independent of the library) for depths up to 8 and
against pngread_util.decode_rgba16 for 16-bit files. Crafted files (pngread_util) choose the
filter type of every row, the deflate level and the IDAT split, so that every path of the
un-filter kernel (all five types, every unit width, the hand-over between bands of 64 rows) and
of the inflate (stored / fixed / dynamic blocks, matches beyond the LDS ring) is decoded."""
import os
import struct
import zlib

import numpy as np
import pytest

from conftest import GOLDEN
import imagecodecs_amd as icx
import pngutil as P
import pngread_util as R

pytestmark = pytest.mark.gpu

REF_PNG = os.path.join(GOLDEN, "png", "test.png")  # the reference's data/test.png


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def decode_ok(ctx, png):
    code, w, h, px = ctx.png_decode(png)
    assert code == icx.PNGR_OK, code
    assert px.shape == (h, w, 4) and px.dtype == np.uint8
    return px


def check(ctx, png, want=None):
    want = R.oracle(png) if want is None else want
    np.testing.assert_array_equal(decode_ok(ctx, png), want)


# ------------------------------------------------------------------ the encoder's own files
def _palette_img(rng, n, w, h, alpha=False):
    pal = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    if not alpha:
        pal[:, 3] = 255
    idx = rng.integers(0, n, (h, w))
    idx.reshape(-1)[:n] = np.arange(n)  # every entry is used
    return pal[idx]


# case -> (colour type, bit depth, tRNS chunk present) lodepng picks for it
OWN = {"grey1": (0, 1, False), "grey2": (0, 2, False), "grey4": (0, 4, False), "grey8": (0, 8, False),
       "pal2": (3, 1, False), "pal4": (3, 2, False), "pal16": (3, 4, False), "pal60": (3, 8, False),
       "pal2_alpha": (3, 1, True), "pal4_alpha": (3, 2, True), "pal16_alpha": (3, 4, True), "pal60_alpha": (3, 8, True),
       "key_grey": (0, 8, True), "key_rgb": (2, 8, True), "grey_alpha": (4, 8, False), "rgb": (2, 8, False),
       "rgba": (6, 8, False)}


def _own_image(case, w, h):
    rng = np.random.default_rng(sorted(OWN).index(case) + 100)
    if case in ("grey1", "grey2", "grey4", "grey8"):
        levels = {"grey8": 256, "grey1": 2, "grey2": 4, "grey4": 16}[case]
        g = (rng.integers(0, levels, (h, w, 1)) * (255 // (levels - 1))).astype(np.uint8)
        return np.repeat(g, 3, axis=2)
    if case.startswith("pal"):
        return _palette_img(rng, int(case[3:].split("_")[0]), w, h, alpha=case.endswith("_alpha"))
    if case == "key_rgb":
        px = P.synth_rgba(5, w, h, opaque=True)
        px[..., :3][(px[..., :3] == (9, 9, 9)).all(axis=2)] = 10
        px[3:6, 4:9] = (9, 9, 9, 0)
        return px
    if case == "key_grey":
        g = rng.integers(0, 256, (h, w, 1)).astype(np.uint8)
        g[g == 77] = 78
        px = np.concatenate([np.repeat(g, 3, axis=2), np.full((h, w, 1), 255, np.uint8)], axis=2)
        px[2:4, 2:4] = (77, 77, 77, 0)
        return px
    if case == "grey_alpha":
        g = rng.integers(0, 256, (h, w, 1)).astype(np.uint8)
        return np.concatenate([np.repeat(g, 3, axis=2), rng.integers(0, 256, (h, w, 1)).astype(np.uint8)], axis=2)
    if case == "rgb":
        return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    return rng.integers(0, 256, (h, w, 4)).astype(np.uint8)


@pytest.mark.parametrize("case", sorted(OWN))
def test_reads_back_what_the_encoder_writes(ctx, case):
    px = np.ascontiguousarray(_own_image(case, 37, 19))
    png = ctx.png_encode(37, 19, px.shape[2], px.tobytes())
    I = P.info(png)
    assert (I["colortype"], I["bitdepth"], I["trns"] is not None) == OWN[case]  # (the mode this case is here for)
    np.testing.assert_array_equal(decode_ok(ctx, png), P.to_rgba(px))


# ------------------------------------------------------------------ every filter, every unit width
MODES = {"grey8": (8, 0), "greyalpha8": (8, 4), "rgb8": (8, 2), "rgba8": (8, 6), "rgb16": (16, 2), "rgba16": (16, 6),
         "grey1": (1, 0), "pal4": (4, 3)}  # bw 1, 2, 3, 4, 6, 8, and two sub-byte forms
SHAPES = [(1, 1), (1, 70), (70, 1), (5, 200), (97, 65), (300, 70)]
PLTE16 = bytes((i * 37 + 11) & 255 for i in range(48))


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_filter_type(ctx, mode, w, h):
    bd, ct = MODES[mode]
    rng = np.random.default_rng(w * 1000 + h + bd * 7 + ct)
    s = R.random_samples(rng, w, h, bd, ct)
    kw = {"plte": PLTE16} if ct == 3 else {}
    want = None
    for kind in (0, 1, 2, 3, 4, "cycle"):
        png = R.make_png(s, bd, ct, types=R.filter_types(kind, h), **kw)
        o = R.oracle(png)
        if want is None:
            want = o
        assert np.array_equal(o, want)  # (the crafted files hold the same pixels under every filter)
        np.testing.assert_array_equal(decode_ok(ctx, png), want, err_msg=f"filter {kind}")


@pytest.mark.parametrize("row64", [2, 3, 4])
@pytest.mark.parametrize("mode", ["rgb8", "rgba16", "grey1"])
def test_band_handover_rows_63_and_64(ctx, mode, row64):
    """Row 64 is the second band's first row: its row above was stored by the first band."""
    bd, ct = MODES[mode]
    w, h = 97, 66
    s = R.random_samples(np.random.default_rng(row64 * 10 + bd), w, h, bd, ct)
    types = [4] * 64 + [row64, 4]
    check(ctx, R.make_png(s, bd, ct, types=types))


# ------------------------------------------------------------------ deflate forms
def _btype(z):
    return (z[2] >> 1) & 3


def test_stored_blocks(ctx):
    s = R.random_samples(np.random.default_rng(5), 61, 33, 8, 2)
    png = R.make_png(s, 8, 2, types=R.filter_types("cycle", 33), level=0)
    assert _btype(P.info(png)["idat"]) == 0
    check(ctx, png)


def test_fixed_huffman_block(ctx):
    s = R.random_samples(np.random.default_rng(6), 7, 5, 8, 0, top=64)  # 5 * (1 + 7) = 40 filtered bytes
    png = R.make_png(s, 8, 0, level=1)
    assert _btype(P.info(png)["idat"]) == 1
    check(ctx, png)


def test_dynamic_block(ctx):
    s = R.random_samples(np.random.default_rng(7), 120, 40, 8, 6, top=40)
    png = R.make_png(s, 8, 6, types=R.filter_types("cycle", 40), level=9)
    assert _btype(P.info(png)["idat"]) == 2
    check(ctx, png)


@pytest.fixture(scope="module")
def far_match():
    """5000 x 6 RGBA, six identical random rows, filter None, level 9: every row after the first is
    copied from 20001 bytes back, past the inflate's 16 KiB ring."""
    row = R.random_samples(np.random.default_rng(8), 5000, 1, 8, 6)
    s = np.repeat(row, 6, axis=0)
    z = zlib.compress(R.forward_filter(R.pack_rows(s, 8), 4, [0] * 6), 9)
    assert len(z) < 30000  # (120006 bytes: the far copies are taken)
    want = s.astype(np.uint8)
    return z, want


@pytest.mark.parametrize("split", [0, 7, 1])
def test_matches_beyond_the_ring_and_split_idat(ctx, far_match, split):
    """split 7 / 1: the zlib stream is cut everywhere, also inside its two header bytes."""
    z, want = far_match
    check(ctx, R.wrap(5000, 6, 8, 6, z, split=split), want)


# ------------------------------------------------------------------ tRNS and palettes
@pytest.mark.parametrize("mode,bd,ct", [("grey8", 8, 0), ("grey16", 16, 0), ("rgb8", 8, 2), ("rgb16", 16, 2), ("grey2", 2, 0)])
def test_trns_key(ctx, mode, bd, ct):
    rng = np.random.default_rng(bd + ct)
    w, h = 23, 11
    s = R.random_samples(rng, w, h, bd, ct)
    key = s[4, 5].copy()
    if bd == 16:
        key[:] = [0x1234, 0xABCD, 0x00FF][: len(key)]
        s[4, 5] = key
        s[2, 3] = key
        s[6, 7] = key ^ 0x0001  # the high bytes match, the low byte does not: opaque
        s[1, 1] = key
        s[1, 1, -1] ^= 0x0100
    trns = b"".join(struct.pack(">H", int(k)) for k in key)
    png = R.make_png(s, bd, ct, types=R.filter_types("cycle", h), trns=trns)
    want = R.oracle(png)
    assert want[4, 5, 3] == 0 and (want[..., 3] == 255).any()
    if bd == 16:
        assert want[6, 7, 3] == 255 and want[1, 1, 3] == 255 and want[2, 3, 3] == 0
    check(ctx, png, want)


def test_short_trns_and_index_past_plte(ctx):
    rng = np.random.default_rng(11)
    w, h = 29, 13
    s = R.random_samples(rng, w, h, 4, 3)  # indices 0..15
    plte = bytes(rng.integers(0, 256, 30, dtype=np.uint8))  # 10 entries
    trns = bytes([0, 128, 7])                               # alpha for the first three
    png = R.make_png(s, 4, 3, types=R.filter_types("cycle", h), plte=plte, trns=trns)
    pal = np.zeros((16, 4), np.uint8)
    pal[:, 3] = 255
    pal[:10, :3] = np.frombuffer(plte, np.uint8).reshape(10, 3)
    pal[:3, 3] = [0, 128, 7]
    want = pal[s[..., 0]]
    assert (s >= 10).any()
    check(ctx, png, want)
    s8 = R.random_samples(rng, w, h, 8, 3)  # 8-bit indices up to 255 with the same 10-entry PLTE
    pal8 = np.zeros((256, 4), np.uint8)
    pal8[:, 3] = 255
    pal8[:16] = pal
    check(ctx, R.make_png(s8, 8, 3, plte=plte, trns=trns), pal8[s8[..., 0]])


# ------------------------------------------------------------------ the reference's file
def test_reference_png(ctx):
    data = open(REF_PNG, "rb").read()
    check(ctx, data, P.decode_rgba(data))


def test_reference_png_equals_pil(ctx):
    Image = pytest.importorskip("PIL.Image")
    want = np.asarray(Image.open(REF_PNG).convert("RGBA"))
    check(ctx, open(REF_PNG, "rb").read(), want)


# ------------------------------------------------------------------ bad data
FLIP_AT = 4242  # the middle byte of the level-9 stream below (8485 bytes with zlib 1.2.11): a dynamic block's symbols.
                # CPU zlib rejects the stream with bit 4 of that byte flipped ("incorrect data check"); the position
                # was found on the CPU, and _bad_files asserts the rejection again wherever it runs


def _bad_files():
    rng = np.random.default_rng(21)
    w, h = 64, 48
    s = R.random_samples(rng, w, h, 8, 6, top=24)
    lb, bw = R.geometry(w, 8, 6)
    raw = R.forward_filter(R.pack_rows(s, 8), bw, R.filter_types("cycle", h))
    z = zlib.compress(raw, 9)
    assert _btype(z) == 2 and len(z) > FLIP_AT + 1000
    flipped = bytearray(z)
    flipped[FLIP_AT] ^= 0x10
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(flipped))
    bad_filter = R.filter_types("cycle", h)
    bad_filter[17] = 5
    return {
        "cut by 5 bytes": R.wrap(w, h, 8, 6, z[:-5]),
        "flipped byte": R.wrap(w, h, 8, 6, bytes(flipped)),
        "filter byte 5": R.make_png(s, 8, 6, types=bad_filter),
        "one row short": R.wrap(w, h, 8, 6, zlib.compress(raw[: -(1 + lb)], 9)),
        "one row long": R.wrap(w, h, 8, 6, zlib.compress(raw + raw[-(1 + lb):], 9)),
        "one byte": R.wrap(w, h, 8, 6, z[:1]),
        "good": R.wrap(w, h, 8, 6, z),
    }


@pytest.mark.parametrize("name", ["cut by 5 bytes", "flipped byte", "filter byte 5", "one row short", "one row long", "one byte"])
def test_bad_data(ctx, name):
    files = _bad_files()
    assert ctx.png_decode(files[name]) == (icx.PNGR_BAD_DATA, 0, 0, None)
    check(ctx, files["good"])  # (and the context decodes the undamaged file afterwards)


# ------------------------------------------------------------------ the batch
def _run_batch(b, files, max_w, max_h, stream_obj=None, misalign=4):
    import torch
    dev = torch.device("cuda", 0)
    n = len(files)
    sizes = np.array([len(f) for f in files], np.uint64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    stride = 4 * max_w * max_h + misalign  # (odd images start 4-, not 16-byte aligned)
    s = stream_obj if stream_obj is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        data = torch.from_numpy(np.frombuffer(b"".join(files), np.uint8).copy()).to(dev)
        d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_sz = torch.from_numpy(sizes.view(np.int64)).to(dev)
        out = torch.full((n * stride,), 0xAB, dtype=torch.uint8, device=dev)
        st = torch.full((n,), -9, dtype=torch.int32, device=dev)
        dims = torch.full((n, 3), -9, dtype=torch.int32, device=dev)
        # (stream 0 means the context's own stream, which is not torch's: the inputs are complete
        # before the call and the whole device is waited for after it)
        torch.cuda.synchronize(dev)
        b.decode_device(n, data.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), out.data_ptr(), stride,
                        st.data_ptr(), dims.data_ptr(), s.cuda_stream)
        torch.cuda.synchronize(dev)
    return st.cpu().numpy(), dims.cpu().numpy(), out.cpu().numpy().reshape(n, stride)


def _batch_files(seed):
    rng = np.random.default_rng(seed)
    mk = lambda w, h, bd, ct, **kw: R.make_png(R.random_samples(rng, w, h, bd, ct), bd, ct,
                                               types=R.filter_types("cycle", h), **kw)
    bad = _bad_files()
    files = [mk(40, 30, 8, 6), mk(1, 1, 16, 2), bad["flipped byte"], mk(64, 48, 4, 3, plte=PLTE16), mk(33, 48, 8, 4),
             mk(65, 10, 8, 2), bad["filter byte 5"], mk(64, 47, 16, 6, split=5), mk(13, 48, 1, 0)]  # 65 > max_w
    codes = [icx.PNGR_OK, icx.PNGR_OK, icx.PNGR_BAD_DATA, icx.PNGR_OK, icx.PNGR_OK, icx.PNGR_TOO_LARGE, icx.PNGR_BAD_DATA,
             icx.PNGR_OK, icx.PNGR_OK]
    if seed & 1:  # a different mix, in another order
        files, codes = files[::-1] + [b"not a png at all"], codes[::-1] + [icx.PNGR_NOT_PNG]
        files, codes = files[1:], codes[1:]
    return files, codes


def _check_batch(res, files, codes):
    st, dims, out = res
    assert list(st) == codes
    for i, (f, c) in enumerate(zip(files, codes)):
        if c != icx.PNGR_OK:
            assert list(dims[i]) == [0, 0, 0]
            continue
        want = R.oracle(f)
        h, w, _ = want.shape
        assert list(dims[i]) == [w, h, 4]
        np.testing.assert_array_equal(out[i, : 4 * w * h].reshape(h, w, 4), want, err_msg=f"image {i}")
        assert (out[i, 4 * w * h:] == 0xAB).all()  # nothing written past the image


def test_batch(ctx):
    import torch
    b = icx.PngBatch(ctx, 9, 64, 48)
    files, codes = _batch_files(2)
    assert len(files) == 9
    _check_batch(_run_batch(b, files, 64, 48), files, codes)
    assert list(b.stage_times()) == ["parse", "gather", "inflate", "unfilter", "expand"]
    files2, codes2 = _batch_files(3)  # the same batch object again, a different mix
    _check_batch(_run_batch(b, files2, 64, 48, misalign=16), files2, codes2)
    side = torch.cuda.Stream(torch.device("cuda", 0))  # and on a stream that is not the default one
    _check_batch(_run_batch(b, files[:5], 64, 48, stream_obj=side), files[:5], codes[:5])
    b.close()


# ------------------------------------------------------------------ Image
def test_image_read_png(tmp_path):
    img = icx.Image()
    img.read(REF_PNG)
    want = P.decode_rgba(open(REF_PNG, "rb").read())
    assert (img.cols(), img.rows(), img.channels(), img.type()) == (499, 289, 4, icx.Image.UBYTE)
    assert img.data().dtype == np.uint8 and img.data().ndim == 1
    assert img.data().tobytes() == want.tobytes()
    bad = tmp_path / "damaged.PNG"
    bad.write_bytes(_bad_files()["cut by 5 bytes"])
    with pytest.raises(RuntimeError, match="Could not read image data"):
        img.read(str(bad))
    hdr = tmp_path / "header.png"
    hdr.write_bytes(b"\x89PNG\r\n\x1a\n" + b"\0" * 40)
    with pytest.raises(RuntimeError, match="Could not read image data"):
        img.read(str(hdr))
