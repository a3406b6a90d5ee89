"""GPU DDS read and write (Image::readDds / writeDds; contract in include/icx.h) against the
restatement in tests/ddsutil.py and the reference's data/test.dds.

Read: status, size, channels, type and every output byte of every file of the shared case lists equal
the restatement's, through Context.dds_decode and through DdsBatch; slots of failed images and the
bytes of a slot past its image stay as they were. Write: the bytes equal the restatement's, RAW and
BC, through dds_save_to_memory and dds_encode_device_batch."""
import os

import numpy as np
import pytest

import imagecodecs_amd as icx
import ddsutil as D

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = open(os.path.join(GOLDEN, "dds", "test.dds"), "rb").read()
KDDS_SEG = 1024  # icx_dds.hip kDdsSeg: pixels per row segment, 256 blocks of 4
STAGES = {"parse", "blocks", "raw"}
WAVE_EDGE_WIDTHS = list(range(1, 10)) + list(range(253, 262)) + list(range(509, 518))


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def _same(got, ref, name=""):
    assert got[0] == ref[0], (name, got[0], ref[0])
    if ref[0] == D.OK:
        assert got[1:5] == ref[1:5], (name, got[1:5], ref[1:5])
        assert got[5].dtype == ref[5].dtype and got[5].tobytes() == ref[5].tobytes(), name  # (bytes: NaN payloads count)
    else:
        assert got[1:5] == (0, 0, 0, 0) and got[5] is None, name


def _batch(ctx, files, max_w, max_h, stride, gaps=None):
    """One icx_dds_batch_decode over `files` (gaps[i] bytes in front of file i) -> per-image (code, w,
    h, d, type, elements or None), stage times. The guard bytes around the slots, the whole slot of
    a failed image and the bytes of a slot past its image must come back untouched."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(files)
    gaps = gaps or [0] * n
    blob, offs = bytearray(), []
    for g, f in zip(gaps, files):
        blob += b"\xEE" * g
        offs.append(len(blob))
        blob += f
    data = torch.from_numpy(np.frombuffer(bytes(blob) or b"\0", np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(np.array(offs, np.int64)).to(dev)
    d_sz = torch.from_numpy(np.array([len(f) for f in files], np.int64)).to(dev)
    assert stride % 16 == 0
    guard = 256
    out = torch.full((guard + n * stride + guard,), 0xA5, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    dims = torch.full((n, 4), -9, dtype=torch.int32, device=dev)
    b = icx.DdsBatch(ctx, n, max_w, max_h)
    stream = torch.cuda.current_stream(dev).cuda_stream
    torch.cuda.synchronize(dev)  # (the fills above are done before another stream writes)
    rc = b.decode_device(n, data.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), out.data_ptr() + guard, stride,
                         st.data_ptr(), dims.data_ptr(), stream)
    assert rc == icx.DDS_OK
    torch.cuda.synchronize(dev)
    times = b.stage_times()
    b.close()
    out, st, dims = out.cpu().numpy(), st.cpu().numpy(), dims.cpu().numpy()
    assert (out[:guard] == 0xA5).all() and (out[-guard:] == 0xA5).all()
    res = []
    for i in range(n):
        w, h, d, t = (int(v) for v in dims[i])
        slot = out[guard + i * stride: guard + (i + 1) * stride]
        arr = None
        if st[i] == icx.DDS_OK:
            nb = w * h * d * (1, 2, 4)[t]
            arr = slot[:nb].view(D.DTYPES[t]).reshape(h, w, d)
            assert (slot[nb:] == 0xA5).all(), f"image {i} wrote past its elements"
        else:
            assert (slot == 0xA5).all(), f"failed image {i} wrote to its slot"
        res.append((int(st[i]), w, h, d, t, arr))
    return res, times


def _check_batch(ctx, cases, gaps=None, pad=16):
    """The cases in one batch whose maxima and slot are the largest image's (+ pad bytes of slot)."""
    refs = [D.decode(f) for _, f in cases]
    ok = [r for r in refs if r[0] == D.OK]
    max_w, max_h = max([r[1] for r in ok] + [1]), max([r[2] for r in ok] + [1])
    stride = (max([r[5].nbytes for r in ok] + [16]) + 15) // 16 * 16 + pad
    res, times = _batch(ctx, [f for _, f in cases], max_w, max_h, stride, gaps)
    for (name, _), got, ref in zip(cases, res, refs):
        _same(got, ref, name)
    return times


def _corpus():
    files = [("fixture", FIXTURE)] + D.block_cases() + D.alias_cases() + D.mask_cases() + D.field_sweep_cases()
    files += [(n, f) for n, f, _ in D.error_cases() if len(f) < 1 << 20]
    return files


# ------------------------------------------------------------------------------------ read
def test_dds_fixture(ctx):
    got = ctx.dds_decode(FIXTURE)
    assert got[:5] == (icx.DDS_OK, 499, 289, 3, icx.PNM_UBYTE)
    ppm = open(os.path.join(GOLDEN, "pnm", "test.ppm"), "rb").read()
    assert got[5].tobytes() == ppm[-499 * 289 * 3:]
    _same(got, D.decode(FIXTURE))


def test_dds_corpus_single_decode(ctx):
    """The one-image entry on every form: aliases, masks, copied forms, every status, and the block
    formats at the sizes around one and two blocks."""
    cases = D.alias_cases() + D.mask_cases() + [(n, f) for n, f, _ in D.error_cases() if len(f) < 1 << 20]
    cases += [(n, f) for n, f in D.block_cases() if n.split("_")[1] in ("1x1", "4x4", "5x5", "21x9", "3x7", "8x1")]
    for name, f in cases:
        _same(ctx.dds_decode(f), D.decode(f), name)


def test_dds_corpus_batch(ctx):
    """The same corpus in batches: the small files in one, the fixture and the field sweeps in another."""
    small = [(n, f) for n, f in _corpus() if D.decode(f)[0] != D.OK or D.decode(f)[5].nbytes <= 4096]
    large = [(n, f) for n, f in _corpus() if D.decode(f)[0] == D.OK and D.decode(f)[5].nbytes > 4096]
    assert len(small) > 1100 and {n for n, _ in large} >= {"fixture", "sweep_r5g6b5", "sweep_a8l8"}
    assert set(_check_batch(ctx, small)) == STAGES
    _check_batch(ctx, large)


def test_dds_prefixes_and_bit_flips(ctx):
    """Every prefix of a DXT5 file, 300 of the fixture's, and 200 seeded bit flips of each."""
    for k, src in enumerate(D.fuzz_sources(FIXTURE)):
        _check_batch(ctx, [(f"prefix{k}_{len(p)}", p) for p in D.prefixes(src)])
        flips = [(f"flip{k}_{j}", p) for j, p in enumerate(D.bit_flips(src, 77 + k))]
        ok = [(n, f) for n, f in flips if D.decode(f)[0] != D.OK or D.decode(f)[5].nbytes <= 4 * 499 * 289 * 2]
        assert len(flips) == 200 and len(ok) >= 190  # (a flipped size bit can ask for a slot of its own size)
        _check_batch(ctx, ok)


@pytest.mark.parametrize("cc", D.BLOCK_FOURCCS, ids=lambda c: c.decode())
def test_dds_blocks_at_wave_edges(ctx, cc):
    """Widths 1-9, 253-261 and 509-517 x heights 1-9: partial blocks, and the 64th and 128th block of
    a row on either side of a wave's edge whatever the lane-to-block mapping."""
    cases = [(f"{w}x{h}", D.block_file(7 * w + h, cc, w, h)) for h in range(1, 10) for w in WAVE_EDGE_WIDTHS]
    assert len(cases) == 27 * 9
    _check_batch(ctx, cases)


def test_dds_rows_longer_than_a_segment(ctx):
    """1030 x 13: a second segment of a block row (KDDS_SEG pixels to a segment), every block format
    and the masked and copied forms; and 1025, 2049 and 4097 pixels, one block or pixel into a segment."""
    assert KDDS_SEG < 1030
    cases = [(f"{cc.decode()}_1030x13", D.block_file(3, cc, 1030, 13)) for cc in D.BLOCK_FOURCCS]
    cases += [(f"{cc.decode()}_{w}x5", D.block_file(w, cc, w, 5)) for cc in (b"DXT1", b"DXT5") for w in (1025, 2049, 4097)]
    cases += [("rgb24_1030x13", D.masked_file(4, 1030, 13, 24, (0xFF0000, 0xFF00, 0xFF, 0))),
              ("bgra_1030x13", D.masked_file(5, 1030, 13, 32, (0xFF0000, 0xFF00, 0xFF, 0xFF000000))),
              ("565_1025x3", D.masked_file(6, 1025, 3, 16, (0xF800, 0x7E0, 0x1F, 0))),
              ("l8_2049x2", D.masked_file(7, 2049, 2, 8, (0xFF, 0, 0, 0), 0x20000)),
              ("float4_1030x3", D.copy_file(8, 1030, 3, dxgi=2, nan=True)), ("ushort1_1025x3", D.copy_file(9, 1025, 3, dxgi=56))]
    _check_batch(ctx, cases)


@pytest.mark.parametrize("form", ["rgb24", "dxt1", "dxt5", "float3"])
def test_dds_every_offset_residue(ctx, form):
    """A file at every d_offsets residue mod 16: the loads are aligned 16-byte loads whatever the offset."""
    make = {"rgb24": lambda k: D.masked_file(k, 37, 5, 24, (0xFF0000, 0xFF00, 0xFF, 0)), "dxt1": lambda k: D.block_file(k, b"DXT1", 70, 9),
            "dxt5": lambda k: D.block_file(k, b"DXT5", 70, 9), "float3": lambda k: D.copy_file(k, 9, 4, dxgi=6)}[form]
    cases = [(f"{form}_res{r}", make(50 + r)) for r in range(16)]
    # file i starts at residue i: the files' lengths are what they are, the gaps make up for them
    gaps, at = [], 0
    for r, (_, f) in enumerate(cases):
        g = (r - at) % 16
        gaps.append(g)
        at += g + len(f)
    _check_batch(ctx, cases, gaps)


def test_dds_batch_mixed(ctx):
    """All forms in one call with failed files between good ones: each image has its own status, a
    failed image's slot and the bytes past an image's end inside its slot are untouched."""
    good = D.alias_cases() + D.mask_cases()[::3] + D.block_cases()[::97]
    bad = [(n, f) for n, f, c in D.error_cases() if c != D.OK and len(f) < 1 << 20]
    cases = []
    for k, g in enumerate(good):
        cases += [g, bad[(2 * k) % len(bad)], bad[(2 * k + 1) % len(bad)]]
    assert sum(D.decode(f)[0] == D.OK for _, f in cases) == len(good) >= 50
    assert set(_check_batch(ctx, cases, pad=48)) == STAGES


def test_dds_misaligned_output_is_refused(ctx):
    import torch
    dev = torch.device("cuda", 0)
    f = D.block_file(1, b"DXT1", 8, 8)
    data = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).to(dev)
    off = torch.zeros(1, dtype=torch.int64, device=dev)
    sz = torch.full((1,), len(f), dtype=torch.int64, device=dev)
    out = torch.full((1024,), 0xA5, dtype=torch.uint8, device=dev)
    st = torch.full((1,), -9, dtype=torch.int32, device=dev)
    dims = torch.full((4,), -9, dtype=torch.int32, device=dev)
    b = icx.DdsBatch(ctx, 1, 8, 8)
    for delta, stride in ((1, 256), (8, 256), (0, 200), (0, 264), (4, 196)):
        rc = b.decode_device(1, data.data_ptr(), off.data_ptr(), sz.data_ptr(), out.data_ptr() + delta, stride, st.data_ptr(),
                             dims.data_ptr())
        assert rc == icx.DDS_INVALID_ARGUMENT, (delta, stride)
    torch.cuda.synchronize(dev)
    assert (out.cpu().numpy() == 0xA5).all() and int(st.cpu()[0]) == -9
    assert b.decode_device(1, data.data_ptr(), off.data_ptr(), sz.data_ptr(), out.data_ptr() + 16, 256, st.data_ptr(),
                           dims.data_ptr()) == icx.DDS_OK
    torch.cuda.synchronize(dev)
    b.close()
    assert int(st.cpu()[0]) == icx.DDS_OK and (out.cpu().numpy()[16:16 + 192] == D.decode(f)[5].reshape(-1)).all()


def test_dds_too_large_for_the_maxima_or_the_slot(ctx):
    wide = D.block_file(1, b"DXT1", 33, 4)
    tall = D.masked_file(2, 8, 21, 24, (0xFF0000, 0xFF00, 0xFF, 0))
    fat = D.copy_file(3, 32, 20, dxgi=2)       # 16 bytes a pixel: inside the maxima, larger than the slot
    ok = D.block_file(4, b"DXT5", 32, 20)      # 4 bytes a pixel: fills the slot exactly
    ok2 = D.copy_file(5, 16, 10, dxgi=2)
    res, _ = _batch(ctx, [wide, ok, tall, fat, ok2], 32, 20, 32 * 20 * 4)
    for k in (0, 2, 3):
        assert res[k][:5] == (icx.DDS_TOO_LARGE, 0, 0, 0, 0), k
    _same(res[1], D.decode(ok))
    _same(res[4], D.decode(ok2))
    _same(ctx.dds_decode(fat), D.decode(fat))  # (the one-image entry sizes its slot by the file)


# ------------------------------------------------------------------------------------ write
def _encode_batch(ctx, imgs, d, fmt, stride=None, pad=3):
    """One dds_encode_device_batch over images of d channels -> (files, sizes, status); the bytes of
    each slot past its file must come back untouched."""
    import torch
    dev = torch.device("cuda", 0)
    srcs = [torch.from_numpy(np.ascontiguousarray(p).copy()).to(dev) for p in imgs]
    stride = stride or max(D.encode_bound(p.shape[1], p.shape[0], d, fmt) for p in imgs) + pad
    n = len(imgs)
    out = torch.full((n * stride + 64,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = torch.zeros((n,), dtype=torch.int64, device=dev)
    status = torch.full((n,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)  # (the fills above are done before the context's stream writes)
    rc = ctx.dds_encode_device_batch([s.data_ptr() for s in srcs], [p.shape[1] for p in imgs], [p.shape[0] for p in imgs], d, fmt,
                                     out.data_ptr(), stride, sizes.data_ptr(), status.data_ptr())
    assert rc == icx.DDS_OK
    out, sizes, status = out.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy()
    files = []
    for i in range(n):
        slot = out[i * stride:(i + 1) * stride]
        k = int(sizes[i]) if status[i] == icx.DDS_OK else 0
        assert (slot[k:] == 0xA5).all(), i
        files.append(slot[:k].tobytes())
    assert (out[n * stride:] == 0xA5).all()
    return files, sizes, status


@pytest.mark.parametrize("fmt", [D.RAW, D.BC], ids=["raw", "bc"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_dds_encode_bytes(ctx, d, fmt):
    """The encoder corpus (noise, flat and two-colour blocks, gradients, crafted ties, widths and
    heights 1-9) in one device batch at an odd stride, and one by one through dds_save_to_memory."""
    imgs = D.encoder_images(d)
    files, sizes, status = _encode_batch(ctx, [p for _, p in imgs], d, fmt)
    for (name, px), f, s in zip(imgs, files, status):
        assert s == icx.DDS_OK and f == D.encode(px, fmt), (name, d, fmt)
    for name, px in imgs[:8] + imgs[8::11]:
        code, data = ctx.dds_save_to_memory(px, fmt)
        assert code == icx.DDS_OK and data == D.encode(px, fmt), (name, d, fmt)
        assert len(data) == icx.dds_encode_bound(px.shape[1], px.shape[0], d, fmt)


def test_dds_encode_exhaustive_alpha(ctx):
    """Every pair a1 < a0 with every value strictly between them, as one d = 1 image of 2048 x 1664."""
    px = D.alpha_exhaustive_image()
    code, data = ctx.dds_save_to_memory(px, icx.DDS_BC)
    assert code == icx.DDS_OK and data == D.encode(px, D.BC)


@pytest.mark.parametrize("fmt", [D.RAW, D.BC], ids=["raw", "bc"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_dds_encode_at_wave_edges(ctx, d, fmt):
    """Widths 253-261 and 509-517 x heights 1-9, the pixels at odd device addresses by their sizes."""
    imgs = [D.synth(w + 31 * h, w, h, d) for h in range(1, 10) for w in WAVE_EDGE_WIDTHS[9:]]
    files, _, status = _encode_batch(ctx, imgs, d, fmt, pad=5)
    for px, f, s in zip(imgs, files, status):
        assert s == icx.DDS_OK and f == D.encode(px, fmt), (px.shape, d, fmt)


@pytest.mark.parametrize("fmt", [D.RAW, D.BC], ids=["raw", "bc"])
def test_dds_encode_rows_longer_than_a_segment(ctx, fmt):
    for d in (1, 2, 3, 4):
        imgs = [D.synth(9 + d, 1030, 13, d), D.synth(3 + d, KDDS_SEG + 1, 2, d), D.synth(4 + d, 2 * KDDS_SEG + 5, 5, d)]
        files, _, status = _encode_batch(ctx, imgs, d, fmt, pad=1)
        for px, f, s in zip(imgs, files, status):
            assert s == icx.DDS_OK and f == D.encode(px, fmt), (px.shape, d, fmt)


@pytest.mark.parametrize("fmt", [D.RAW, D.BC], ids=["raw", "bc"])
def test_dds_encode_too_large_and_bad_sizes(ctx, fmt):
    """A file that does not fit writes nothing and reports the size it needs; a bad width gets
    INVALID_ARGUMENT; the neighbours' files are intact."""
    import torch
    d = 3
    imgs = [D.synth(1, 40, 9, d), D.synth(2, 90, 70, d), D.synth(3, 17, 5, d), D.synth(4, 8, 8, d)]
    stride = D.encode_bound(40, 9, d, fmt) + 7
    assert stride < D.encode_bound(90, 70, d, fmt)
    dev = torch.device("cuda", 0)
    srcs = [torch.from_numpy(p.copy()).to(dev) for p in imgs]
    out = torch.full((4 * stride,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = torch.full((4,), -1, dtype=torch.int64, device=dev)
    status = torch.full((4,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rc = ctx.dds_encode_device_batch([s.data_ptr() for s in srcs], [40, 90, 17, 0], [9, 70, 5, 8], d, fmt, out.data_ptr(), stride,
                                     sizes.data_ptr(), status.data_ptr())
    assert rc == icx.DDS_OK
    out, sizes, status = out.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy()
    assert list(status) == [icx.DDS_OK, icx.DDS_TOO_LARGE, icx.DDS_OK, icx.DDS_INVALID_ARGUMENT]
    assert sizes[1] == D.encode_bound(90, 70, d, fmt) and sizes[3] == 0
    assert (out[stride:2 * stride] == 0xA5).all() and (out[3 * stride:] == 0xA5).all()
    for i in (0, 2):
        want = D.encode(imgs[i], fmt)
        assert sizes[i] == len(want) and out[i * stride:i * stride + len(want)].tobytes() == want
        assert (out[i * stride + len(want):(i + 1) * stride] == 0xA5).all()


def test_dds_encode_bad_arguments(ctx):
    for shape in ((4, 4, 5), (0, 4, 3), (4, 0, 3), (65536, 1, 1), (1, 65536, 1), (2, 2, 2, 2)):
        assert ctx.dds_save_to_memory(np.zeros(shape, np.uint8)) == (icx.DDS_INVALID_ARGUMENT, None), shape
    assert ctx.dds_save_to_memory(np.zeros((4, 4, 3), np.uint8), 2) == (icx.DDS_INVALID_ARGUMENT, None)
    assert ctx.dds_save_to_memory(np.zeros((4, 4, 3), np.uint16)) == (icx.DDS_INVALID_ARGUMENT, None)
    assert ctx.dds_encode_device_batch([1], [4], [4], 5, 0, 1, 100, 1, 1) == icx.DDS_INVALID_ARGUMENT
    assert ctx.dds_encode_device_batch([1], [4], [4], 3, 7, 1, 100, 1, 1) == icx.DDS_INVALID_ARGUMENT
    assert ctx.dds_encode_device_batch([1], [4], [4], 3, 0, 0, 100, 1, 1) == icx.DDS_INVALID_ARGUMENT


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_dds_round_trip_through_the_gpu_read(ctx, d):
    """RAW comes back as the pixels with the same d; BC comes back as the restatement decodes it."""
    px = D.synth(70 + d, 131, 23, d)
    code, raw = ctx.dds_save_to_memory(px, icx.DDS_RAW)
    got = ctx.dds_decode(raw)
    assert code == icx.DDS_OK and got[:5] == (icx.DDS_OK, 131, 23, d, icx.PNM_UBYTE) and (got[5] == px).all()
    code, bc = ctx.dds_save_to_memory(px, icx.DDS_BC)
    assert code == icx.DDS_OK
    _same(ctx.dds_decode(bc), D.decode(D.encode(px, D.BC)))


def test_dds_write_reproduces_the_fixture(ctx):
    px = D.decode(FIXTURE)[5]
    code, data = ctx.dds_save_to_memory(px)
    assert code == icx.DDS_OK and len(data) == len(FIXTURE) and data[128:] == FIXTURE[128:]


# ------------------------------------------------------------------------------------ icx.Image
def test_image_read_dds(tmp_path):
    p = tmp_path / "x.DDS"
    p.write_bytes(FIXTURE)
    img = icx.Image()
    img.read(str(p))
    assert (img.cols(), img.rows(), img.channels(), img.type()) == (499, 289, 3, icx.Image.UBYTE)
    assert img.totalBytes() == 499 * 289 * 3 and img.data().tobytes() == D.decode(FIXTURE)[5].tobytes()
    f = D.copy_file(1, 9, 4, dxgi=6, nan=True)
    (tmp_path / "f.dds").write_bytes(f)
    img.read(str(tmp_path / "f.dds"))
    assert (img.cols(), img.rows(), img.channels(), img.type()) == (9, 4, 3, icx.Image.FLOAT)
    assert img.data().tobytes() == D.decode(f)[5].tobytes()
    none = tmp_path / "none.dds"
    none.write_bytes(b"DDX " + FIXTURE[4:200])
    with pytest.raises(RuntimeError):
        icx.Image().read(str(none))


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_image_write_read_round_trip(tmp_path, d):
    px = D.synth(90 + d, 67, 31, d)
    img = icx.Image()
    img.load(px, 67, 31, d)
    p = tmp_path / f"rt{d}.dds"
    img.write(str(p))
    assert p.read_bytes() == D.encode(px, D.RAW)
    back = icx.Image()
    back.read(str(p))
    assert (back.cols(), back.rows(), back.channels()) == (67, 31, d)
    assert back.data().tobytes() == px.tobytes()


def test_image_write_refuses_other_types(tmp_path):
    """A non-UBYTE image is refused: nothing is thrown, no pixels are written."""
    img = icx.Image()
    img.load(np.zeros(12, np.float32), 2, 2, 3, icx.Image.FLOAT)
    p = tmp_path / "f.dds"
    img.write(str(p))
    assert not p.exists() or p.read_bytes() == b""
