"""GPU GIF read (Image::readGif, codecs.cpp:507-542; contract in include/icx.h) against the serial
restatement in tests/gifutil.py: result code, size and pixels of every file equal the
restatement's exactly -- the reference's data/test.gif, PIL-written files, and the crafted corpus
(code sizes and widths, interlaced heights, width steps and the full table, clears, stream starts
and ends, long strings, sub-block plans, ring staging, containers and palettes, every status)."""
import io
import os

import numpy as np
import pytest

import imagecodecs_amd as icx
import gifutil as G

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = open(os.path.join(GOLDEN, "gif", "test.gif"), "rb").read()
KGIF_WIN = 2048   # icx_gif.hip kGifWin: file bytes per window load of k_gif_lzw
KGIF_RING = 2048  # kGifRing: code bytes its ring holds
KGIF_SEG = 1024   # kGifSeg: pixels per row segment of k_gif_render
STAGES = {"parse", "lzw", "render"}


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def _same(got, data, name="", **limits):
    ref = G.decode(data, **limits)
    assert got[0] == ref[0], (name, got[0], ref[0])
    if ref[0] == G.OK:
        assert got[1:3] == ref[1:3], name
        np.testing.assert_array_equal(got[3], ref[3], err_msg=name)
    else:
        assert got[1:3] == (0, 0) and got[3] is None, name


def _batch(ctx, files, max_w, max_h, pad=0, shift=0):
    """The files in one batch; the first file starts `shift` bytes into the data, slots are
    3 * max_w * max_h + pad bytes apart."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(files)
    sizes = np.array([len(f) for f in files], np.int64)
    offs = np.zeros(n, np.int64)
    offs[1:] = np.cumsum(sizes)[:-1]
    offs += shift
    blob = b"\xEE" * shift + b"".join(files) or b"\0"
    data = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(offs).to(dev)
    d_sz = torch.from_numpy(sizes).to(dev)
    stride = 3 * max_w * max_h + pad
    guard = 256
    out = torch.full((guard + n * stride + guard,), 0xA5, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    dims = torch.full((n, 3), -9, dtype=torch.int32, device=dev)
    b = icx.GifBatch(ctx, n, max_w, max_h)
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
        if st[i] == icx.GIF_OK:
            assert d == 3
            arr = slot[:w * h * 3].reshape(h, w, 3)
            assert (slot[w * h * 3:] == 0xA5).all(), f"image {i} wrote past its pixels"
        else:
            assert (w, h, d) == (0, 0, 0)
        res.append((int(st[i]), w, h, arr))
    return res, times


def _check_batch(ctx, files, max_w, max_h, **kw):
    res, times = _batch(ctx, [f for _, f in files], max_w, max_h, **kw)
    assert set(times) == STAGES
    for (name, f), got in zip(files, res):
        _same(got, f, name, max_w=max_w, max_h=max_h)
    return res


def _pil_files():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2)
    out = []
    for name, arr, kw in (("noise8", rng.integers(0, 256, (97, 131), dtype=np.uint8), {}),
                          ("noise2", rng.integers(0, 4, (64, 65), dtype=np.uint8), {}),
                          ("flat", np.full((70, 300), 7, np.uint8), {}),
                          ("low", rng.integers(0, 16, (3, 9), dtype=np.uint8), {}),
                          ("gradient", (np.add.outer(np.arange(200), np.arange(300)) // 3 % 256).astype(np.uint8), {}),
                          ("not_interlaced", rng.integers(0, 256, (37, 53), dtype=np.uint8), {"interlace": False})):
        im = Image.fromarray(arr, "P")
        im.putpalette(rng.integers(0, 256, 768, dtype=np.uint8).tobytes())
        b = io.BytesIO()
        im.save(b, "GIF", **kw)
        out.append(("pil_" + name, b.getvalue()))
    return out


def test_gif_fixture(ctx):
    got = ctx.gif_decode(FIXTURE)
    assert got[:3] == (icx.GIF_OK, 499, 289)
    _same(got, FIXTURE, "fixture")


def test_gif_pil_written_files(ctx):
    Image = pytest.importorskip("PIL.Image")
    files = _pil_files()
    assert sum(G.parse(f)[1]["interlace"] for _, f in files) >= 4
    for name, data in files:
        got = ctx.gif_decode(data)
        _same(got, data, name)
        np.testing.assert_array_equal(got[3], np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), err_msg=name)


def test_gif_corpus_in_one_batch(ctx):
    """Code sizes x widths, interlaced heights, width steps, the full table, clears, stream starts
    and ends, long strings, sub-block plans, containers and palettes."""
    files = [("fixture", FIXTURE)] + G.corpus()
    assert len(files) > 110
    _check_batch(ctx, files, 499, 289)


def test_gif_corpus_single(ctx):
    """The host in / host out entry on one file of each group."""
    names = dict(G.corpus())
    for name in ("mcs2_w65", "mcs8_w257", "interlaced_h3", "interlaced_h17", "greedy_fill", "clear_at_full", "consecutive_clears",
                 "no_leading_clear", "early_stop", "terminator_mid_image", "kwkwk_across_frame_end", "flat_300x70", "period65",
                 "plan_all_1", "no_global_table", "clipped_interlaced", "transparent_on", "two_gce_last_off", "extensions",
                 "second_frame", "trailer_first", "trailer_first_no_table", "zero_width_frame"):
        _same(ctx.gif_decode(names[name]), names[name], name)


def test_gif_ring_staging(ctx):
    """A stream of more than three windows and three rings, through sub-blocks of 255 and of 1, and
    rows of more than three render segments."""
    idx = G.noise(31, 3, 3 * KGIF_SEG + 77, 256)
    for plan in ((255,), (1,), (7, 255, 1)):
        data = G.simple_gif(idx, G.palette(256, 1), plan=plan)
        stream, end = G.data_stream(data, G.parse(data)[1]["data_at"])
        assert len(stream) > 3 * max(KGIF_WIN, KGIF_RING)
        _same(ctx.gif_decode(data), data, f"plan{plan}")
    cut = data[:len(data) // 2]
    assert G.decode(cut)[0] == G.TRUNCATED
    _same(ctx.gif_decode(cut), cut, "cut")


def test_gif_every_status(ctx):
    cases = G.status_cases()
    assert {c for _, _, c in cases} == {G.OK, G.NOT_GIF, G.BAD_HEADER, G.MALFORMED, G.BAD_DATA, G.TRUNCATED}
    for name, data, want in cases:
        assert G.decode(data)[0] == want, name
        _same(ctx.gif_decode(data), data, name)
    res = _check_batch(ctx, [(n, f) for n, f, _ in cases], 16, 16)
    assert [r[0] for r in res] == [c for _, _, c in cases]


def test_gif_prefixes_and_mutants(ctx):
    """Every prefix of one file and 200 seeded bit flips of it, each at the very end of the data
    buffer or followed by another file: defined statuses, and no read past a file's length can go
    unnoticed in the result."""
    base = G.base_file()
    files = [(f"prefix{k}", base[:k]) for k in range(len(base) + 1)] + G.mutants(base)
    seen = {G.decode(f)[0] for _, f in files}
    assert seen >= {G.OK, G.NOT_GIF, G.BAD_HEADER, G.MALFORMED, G.BAD_DATA, G.TRUNCATED}
    _check_batch(ctx, files, 64, 64)


@pytest.mark.parametrize("shift", [0, 1, 7, 12])
def test_gif_batch_start_residues(ctx, shift):
    """The mixed corpus at four start residues mod 16, slots an odd number of bytes apart:
    sentinel bytes after each slot's pixels stay, failures have zero dims."""
    names = dict(G.corpus())
    files = [(n, names[n]) for n in ("mcs3_w63", "mcs8_w257", "interlaced_h9", "literal_fill_3_to_12", "flat_300x70", "period3",
                                     "plan_random", "sub_rectangle_interlaced", "clipped", "transparent_on", "trailer_first")]
    files += [(n, f) for n, f, _ in G.status_cases()] + [("fixture", FIXTURE)]
    res = _check_batch(ctx, files, 300, 289, pad=1 + shift, shift=shift)
    assert res[-1][0] == G.TOO_LARGE  # the fixture is 499 wide
    assert sum(r[0] != G.OK for r in res) > 10


@pytest.mark.parametrize("pad", [1, 2, 3])
def test_gif_batch_segment_edges(ctx, pad):
    """1 x 1, 5 x 2 and (KGIF_SEG + 1) x 2, twice, the slots' stride padded by 1, 2 or 3 bytes, the data
    an odd number of bytes into the buffer: rows shorter than 16 bytes that start off alignment, a
    ragged head before the 16-byte stores and a tail after them, and a second row segment of one
    pixel; the window load's first and last 16 bytes straddle the file's ends."""
    files = [(f"{w}x{h}", G.simple_gif(G.noise(70 + w, h, w, 256), G.palette(256, 1))) for w, h in ((1, 1), (5, 2), (KGIF_SEG + 1, 2))]
    res = _check_batch(ctx, files + files, KGIF_SEG + 1, 2, pad=pad, shift=2 * pad + 1)
    assert all(r[0] == G.OK for r in res)


def test_gif_too_large(ctx):
    data = G.simple_gif(G.noise(1, 9, 33, 4), G.palette(4))
    for mw, mh, want in ((33, 9, G.OK), (32, 9, G.TOO_LARGE), (33, 8, G.TOO_LARGE)):
        res, _ = _batch(ctx, [data, data], mw, mh)
        assert [r[0] for r in res] == [want, want]
    huge = G.screen(65535, 65535, G.palette(4)) + b";"
    assert ctx.gif_decode(huge)[:3] == (icx.GIF_TOO_LARGE, 0, 0)


def test_gif_image_read(ctx, tmp_path):
    p = tmp_path / "a.GIF"
    p.write_bytes(FIXTURE)
    img = icx.Image()
    img.read(str(p))
    assert (img.cols(), img.rows(), img.channels(), img.type()) == (499, 289, 3, icx.Image.UBYTE)
    np.testing.assert_array_equal(img.data().reshape(289, 499, 3), G.decode(FIXTURE)[3])
    bad = tmp_path / "bad.gif"
    bad.write_bytes(FIXTURE[:2000])
    with pytest.raises(RuntimeError, match="Could not read image data"):
        icx.Image().read(str(bad))
    img.load(np.zeros((4, 4, 3), np.uint8), 4, 4, 3)
    with pytest.raises(ValueError):
        img.write(str(tmp_path / "out.gif"))
