"""GPU GIF write (Image::writeGif; contract in include/icx.h "GIF write") against the restatement in
tests/gifwutil.py: every file equals the restatement's byte for byte, is at most
icx_gif_encode_bound, and reads back through the GPU read -- the batch read, straight from the
device slots the write filled, which runs the kernels of ctx.gif_decode; single files through
ctx.gif_decode itself -- to the restatement's pixels. Every batch has an odd out_stride, odd source
addresses and sentinel bytes around each slot."""
import os

import numpy as np
import pytest

import imagecodecs_amd as icx
import gifutil as G
import gifwutil as W

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENT = 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def _a3(a):
    a = np.ascontiguousarray(a, np.uint8)
    return a[:, :, None] if a.ndim == 2 else a


def _encode(ctx, imgs, seg=0, dither=0, mode=W.AUTO, stride=None, null=(), readback=True):
    """One icx_gif_encode_device_batch -> (rc, status, sizes, files). Sources at odd addresses, an
    odd stride, sentinels before, between (a slot's bytes past its file) and after the slots. With
    readback, the batch read decodes the slots in place to the restatement's pixels."""
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
    bounds = [icx.gif_encode_bound(a.shape[1], a.shape[0], seg) for a in imgs]
    if stride is None:
        stride = max(bounds + [8]) | 1
    out = torch.full((1 + n * stride + 64,), SENT, dtype=torch.uint8, device=dev)
    base = out.data_ptr() + 1
    assert base & 1 and all((src.data_ptr() + o) & 1 for o in offs) and stride & 1
    d_sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
    d_status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ptrs = [0 if i in null else src.data_ptr() + o for i, o in enumerate(offs)]
    rc = ctx.gif_encode_device_batch(ptrs, [a.shape[1] for a in imgs], [a.shape[0] for a in imgs], d, seg, dither, mode,
                                     base, stride, d_sizes.data_ptr(), d_status.data_ptr())
    if rc != icx.GIF_OK:
        return rc, None, None, None
    host = out.cpu().numpy()
    status, sizes = d_status.cpu().numpy(), d_sizes.cpu().numpy()
    files = []
    assert host[0] == SENT and (host[1 + n * stride:] == SENT).all(), "bytes outside the slots changed"
    for i in range(n):
        slot = host[1 + i * stride:1 + (i + 1) * stride]
        if status[i] == icx.GIF_OK:
            assert 0 < sizes[i] <= bounds[i], (i, sizes[i], bounds[i])
            assert (slot[sizes[i]:] == SENT).all(), ("bytes after the file changed", i)
            files.append(slot[:sizes[i]].tobytes())
        else:
            assert (slot == SENT).all(), ("a failed image's slot changed", i, status[i])
            files.append(None)
    if readback and all(f is not None for f in files):
        mw, mh = max(a.shape[1] for a in imgs), max(a.shape[0] for a in imgs)
        gb = icx.GifBatch(ctx, n, mw, mh)
        pstride = (3 * mw * mh + 15) & ~15
        pix = torch.zeros(n * pstride, dtype=torch.uint8, device=dev)
        st = torch.full((n,), -7, dtype=torch.int32, device=dev)
        dims = torch.zeros(3 * n, dtype=torch.int32, device=dev)
        foff = torch.tensor([1 + i * stride for i in range(n)], dtype=torch.int64, device=dev)
        gb.decode_device(n, out.data_ptr(), foff.data_ptr(), d_sizes.data_ptr(), pix.data_ptr(), pstride, st.data_ptr(),
                         dims.data_ptr())
        torch.cuda.synchronize()
        hp, hs, hd = pix.cpu().numpy(), st.cpu().numpy(), dims.cpu().numpy().reshape(n, 3)
        gb.close()
        for i, a in enumerate(imgs):
            assert hs[i] == icx.GIF_OK and tuple(hd[i]) == (a.shape[1], a.shape[0], 3), (i, hs[i], hd[i])
            exp = W.expected_pixels(a, dither, mode)
            np.testing.assert_array_equal(hp[i * pstride:i * pstride + exp.size], exp.reshape(-1), err_msg="read back %d" % i)
    return rc, status, sizes, files


def _run_cases(ctx, cases):
    """Cases grouped by what one call shares (d, segment_pixels, dither, palette_mode): a batch
    each, every file the restatement's."""
    groups = {}
    for case in cases:
        name, a, seg, dither, mode = case
        groups.setdefault((_a3(a).shape[2], seg, dither, mode), []).append(case)
    for (d, seg, dither, mode), group in groups.items():
        rc, status, sizes, files = _encode(ctx, [c[1] for c in group], seg, dither, mode)
        assert rc == icx.GIF_OK and (status == icx.GIF_OK).all(), (d, seg, dither, mode, status)
        for case, f in zip(group, files):
            ref = W.restated(case)
            assert f == ref, (case[0], len(f), len(ref), next((i for i, (x, y) in enumerate(zip(f, ref)) if x != y), None))


@pytest.mark.parametrize("d", (1, 3, 4))
def test_sizes_and_colours(ctx, d):
    """Widths 1-21 x heights 1-9, widths 253-259 and 509-515 x heights 1-3; 1 .. 257 colours; d in
    1, 3, 4; noise, flat and smooth; the cube with and without dither, and forced on 3 colours."""
    assert len(W.grid_cases()) > 300
    cases = [c for c in W.grid_cases() if c[1].shape[2] == d]
    assert len(cases) > 100 and any(c[4] == W.CUBE for c in cases)
    _run_cases(ctx, cases)


def test_segment_ends(ctx):
    """segment_pixels in 64, 65, 255, 4096, 0, -1 with N = k * seg and k * seg + 1."""
    cases = W.segment_end_cases()
    assert {c[2] for c in cases} == set(W.SEGS)
    _run_cases(ctx, cases)


@pytest.mark.parametrize("m", (2, 3, 8))
def test_width_steps_and_stream_ends(ctx, m):
    """The 1 x N images N = 1..600 of noise, whole and in segments of 64: the last code before a
    Clear or the stop code on every side of every width step."""
    imgs = W.row_cases(m)
    assert len(imgs) == 600 and W.quantise(imgs[-1])[3] == m
    for seg in (-1, 64):
        rc, status, sizes, files = _encode(ctx, imgs, seg)
        assert rc == icx.GIF_OK and (status == icx.GIF_OK).all()
        for a, f in zip(imgs, files):
            assert f == W.write_gif(a, seg), (m, a.shape[1], seg)


def test_table_full_clear(ctx):
    """Two fills at m = 8, fills at m = 2, and segments that end 0, 1 and 2 pixels after the pixel
    that filled the table."""
    cases = W.table_full_cases()
    assert len(cases) == 8
    _run_cases(ctx, cases)


def test_sub_block_framing(ctx):
    cases = W.framing_cases()
    assert sorted(int(c[0].split("_")[0][7:]) for c in cases) == [254, 255, 256, 509, 510, 511]
    _run_cases(ctx, cases)
    for case in cases:
        assert W.payload_size(case[1], case[2]) == int(case[0].split("_")[0][7:])


def test_multi_wave(ctx):
    """512 x 512 at the default segment size: four waves' strings merged."""
    case = W.multi_wave_case()[0]
    assert len(W.segment_offsets(case[1], case[2])) == 4
    _run_cases(ctx, [case])


def test_batch_slots_and_codes(ctx):
    """Mixed sizes in one call; TOO_LARGE with d_sizes reporting the need and nothing written; a
    null d_src[i]; a refused size inside a batch."""
    imgs = [W.image(k, h, w, 3, n, kind) for k, (h, w, n, kind) in
            enumerate(((1, 1, 1, "flat"), (40, 300, 200, "noise"), (9, 21, 5, "smooth"), (130, 129, 256, "noise"), (2, 515, 17, "flat")))]
    rc, status, sizes, files = _encode(ctx, imgs, 255)
    assert rc == icx.GIF_OK and (status == icx.GIF_OK).all()
    refs = [W.write_gif(a, 255) for a in imgs]
    assert files == refs
    # an odd stride a byte or two short of the second file
    stride = (len(refs[1]) - 2) | 1
    rc, status, sizes, files = _encode(ctx, imgs, 255, stride=stride, null=(2,), readback=False)
    assert rc == icx.GIF_OK
    for i, ref in enumerate(refs):
        if i == 2:
            assert status[i] == icx.GIF_INVALID_ARGUMENT and sizes[i] == 0 and files[i] is None
        elif len(ref) > stride:
            assert status[i] == icx.GIF_TOO_LARGE and sizes[i] == len(ref) and files[i] is None, (i, status[i], sizes[i])
        else:
            assert status[i] == icx.GIF_OK and files[i] == ref, i
    assert sum(len(r) > stride for r in refs) >= 2 and sum(len(r) <= stride for r in refs) >= 2
    exact = len(refs[3]) | 1  # (the slot may be as long as the file, to the byte when that is odd)
    rc, status, sizes, files = _encode(ctx, imgs[3:4], 255, stride=exact, readback=False)
    assert status[0] == icx.GIF_OK and files[0] == refs[3]


def test_refused_arguments(ctx):
    import torch
    a = W.image(1, 4, 4, 3, 4)
    assert ctx.gif_save_to_memory(a)[0] == icx.GIF_OK
    for kw in (dict(segment_pixels=63), dict(segment_pixels=1), dict(segment_pixels=-2), dict(dither=2), dict(palette_mode=2),
               dict(palette_mode=-1)):
        assert ctx.gif_save_to_memory(a, **kw) == (icx.GIF_INVALID_ARGUMENT, None), kw
    assert ctx.gif_save_to_memory(np.zeros((4, 4, 2), np.uint8))[0] == icx.GIF_INVALID_ARGUMENT
    assert ctx.gif_save_to_memory(np.zeros((4, 4, 3), np.uint16))[0] == icx.GIF_INVALID_ARGUMENT
    assert ctx.gif_save_to_memory(np.zeros((0, 4, 3), np.uint8))[0] == icx.GIF_INVALID_ARGUMENT
    assert ctx.gif_save_to_memory(np.zeros((1, 65536, 1), np.uint8))[0] == icx.GIF_INVALID_ARGUMENT
    # the batch entry: the call's code for what the call shares, the image's for its own size
    for seg, dither, mode in ((63, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, 2)):
        assert _encode(ctx, [a], seg, dither, mode)[0] == icx.GIF_INVALID_ARGUMENT, (seg, dither, mode)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    p, r = buf.data_ptr(), res.data_ptr()
    assert ctx.gif_encode_device_batch([p], [4], [4], 2, 0, 0, 0, p + 1024, 2048, r, r + 8) == icx.GIF_INVALID_ARGUMENT
    assert ctx.gif_encode_device_batch([p], [4], [4], 3, 0, 0, 0, 0, 2048, r, r + 8) == icx.GIF_INVALID_ARGUMENT
    assert ctx.gif_encode_device_batch([p], [4], [4], 3, 0, 0, 0, p + 1024, 2048, 0, r + 8) == icx.GIF_INVALID_ARGUMENT
    assert ctx.gif_encode_device_batch([p], [4], [4], 3, 0, 0, 0, p + 1024, 2048, r, 0) == icx.GIF_INVALID_ARGUMENT
    assert ctx.gif_encode_device_batch([p] * 65536, [4] * 65536, [4] * 65536, 3, 0, 0, 0, p + 1024, 0, r, r + 8) == icx.GIF_INVALID_ARGUMENT
    assert ctx.gif_encode_device_batch([], [], [], 3, 0, 0, 0, 0, 0, 0, 0) == icx.GIF_OK
    for w, h in ((0, 4), (4, 0), (65536, 1), (-3, 4), (32769, 32768)):
        st = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        assert ctx.gif_encode_device_batch([p, p], [w, 4], [h, 4], 3, 0, 0, 0, p + 1024, 1024, r, st.data_ptr()) == icx.GIF_OK
        assert st.cpu().tolist() == [icx.GIF_INVALID_ARGUMENT, icx.GIF_OK] and res.cpu().tolist()[0] == 0, (w, h)


@pytest.mark.parametrize("d", (1, 3, 4))
def test_decode_of_encode_is_identity(ctx, d):
    """256 colours or fewer: ctx.gif_decode(ctx.gif_save_to_memory(x)) is x (without its alpha)."""
    for k, (h, w, n, kind, seg) in enumerate(((1, 1, 1, "flat", 0), (9, 21, 2, "noise", 64), (33, 65, 256, "noise", 255),
                                              (64, 64, 17, "smooth", -1), (3, 515, 129, "noise", 4096))):
        a = W.image(300 + k + d, h, w, d, n, kind)
        code, f = ctx.gif_save_to_memory(a, seg)
        assert code == icx.GIF_OK and f == W.write_gif(a, seg), (d, k)
        code, ww, hh, px = ctx.gif_decode(f)[:4]
        assert (code, ww, hh) == (icx.GIF_OK, w, h)
        np.testing.assert_array_equal(np.asarray(px).reshape(h, w, 3), W.rgb_of(a))


def test_fixture_round_trip(ctx):
    """tests/golden/gif/test.gif read, written back and read again: the same pixels."""
    data = open(os.path.join(GOLDEN, "gif", "test.gif"), "rb").read()
    code, w, h, px = ctx.gif_decode(data)[:4]
    assert code == icx.GIF_OK
    px = np.asarray(px).reshape(h, w, 3)
    for seg, dither in ((0, False), (4096, True)):
        code, f = ctx.gif_save_to_memory(px, seg, dither)
        assert code == icx.GIF_OK and f == W.write_gif(px, seg)  # (256 colours or fewer: dither changes nothing)
        code, w2, h2, px2 = ctx.gif_decode(f)[:4]
        assert (code, w2, h2) == (icx.GIF_OK, w, h)
        np.testing.assert_array_equal(np.asarray(px2).reshape(h, w, 3), px)
    assert G.decode(f)[0] == G.OK


def test_python_image_write_gif(ctx, tmp_path, capsys):
    """Image.writeGif, defaults and explicit arguments, gives the restatement's bytes; another type
    or a refused segment size writes nothing; write(".gif") still raises."""
    a = W.image(8, 11, 23, 3, 40, "noise")
    img = icx.Image()
    img.load(a.reshape(-1), 23, 11, 3)
    p = str(tmp_path / "named.anything")
    img.writeGif(p)
    assert open(p, "rb").read() == W.write_gif(a)
    many = W.many_colours(9, 11, 23, 3)
    img.load(many.reshape(-1), 23, 11, 3)
    img.writeGif(p, 64, True)
    assert open(p, "rb").read() == W.write_gif(many, 64, 1)
    q = str(tmp_path / "u16.gif")
    u = icx.Image()
    u.load(np.zeros(16, np.uint16), 4, 4, 1, icx.Image.USHORT)
    u.writeGif(q)
    assert not os.path.exists(q) and "only UBYTE" in capsys.readouterr().err
    img.writeGif(q, 63)  # a refused segment size: a line, no file
    assert not os.path.exists(q)
    with pytest.raises(ValueError):
        img.write(str(tmp_path / "x.gif"))
