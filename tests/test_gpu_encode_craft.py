"""GPU JPEG encoder against the oracle on the crafted inputs of tests/jpegenc_craft.py: the entropy
coder's extremes (10-bit amplitudes behind 16-bit codes, category-11 DC differences in a run and
across the look-back, three ZRLs, a lone coefficient 63, FF pairs and triples across the stuffing
lanes' and workgroups' edges), every run geometry around the 512-pixel run, the pixel loader's
paths, the batch entry and its output cap. Byte equality everywhere; tests/test_encode_craft.py
asserts (on the CPU) that the inputs reach the states named here."""
import numpy as np
import pytest

import imagecodecs_amd as icx
from oracle import pyoracle as O
import jpegenc_craft as J

pytestmark = pytest.mark.gpu
KINDS = ("tje", 444, 420)


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def oracle(kind, q, px):
    h, w, c = px.shape
    return O.tje_encode(q, w, h, c, px.tobytes()) if kind == "tje" else O.jpeg_encode(q, kind, w, h, c, px.tobytes())


def gpu(ctx, kind, q, px):
    h, w, c = px.shape
    return ctx.tje_encode(q, w, h, c, px.tobytes()) if kind == "tje" else ctx.jpeg_encode(q, kind, w, h, c, px.tobytes())


def roundtrip(ctx, jpg, w, h):
    code, dw, dh, n, dec = ctx.decode(jpg)
    ocode, _, _, _, odec = O.decode(jpg)
    assert (code, ocode) == (0, 0) and (dw, dh, n) == (w, h, 3) and dec == odec


# ---- host entries: every crafted family, every quality, 3 and 4 bytes a pixel; the GPU decoder
# reads back what the GPU encoder wrote (16-bit codes with 10-bit amplitudes, ZRL triples and
# category-11 DC differences through the parallel Huffman decode)
@pytest.mark.parametrize("comps", [3, 4])
@pytest.mark.parametrize("family", J.FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_host_entries_match_oracle_and_roundtrip(ctx, kind, family, comps):
    for fam, name, px in J.crafted(kind, comps):
        if fam != family:
            continue
        h, w, _ = px.shape
        for q in J.QUALITIES[kind]:
            out = gpu(ctx, kind, q, px)
            assert out == oracle(kind, q, px), (name, q)
            if comps == 3:  # (the same file either way)
                roundtrip(ctx, out, w, h)


def test_host_second_pass_and_fresh_words_buffer(ctx):
    """The two noise images by name: noise_big's file exceeds source + 64 KiB, so the host entry's
    first pass only sizes it and the second writes it; noise_small (256 x 64) outgrows the 64 KiB
    words buffer a fresh workspace starts with and is encoded again at its measured size."""
    big, small = J.noise01(*J.NOISE_BIG), J.noise01(*J.NOISE_SMALL)
    for kind, q in (("tje", 3), (444, 100)):
        want = oracle(kind, q, big)
        assert len(want) > big.size + 65536
        assert gpu(ctx, kind, q, big) == want
        want = oracle(kind, q, small)
        assert small.size // 4 < 65536 < len(J.scan_bytes(want))
        assert gpu(ctx, kind, q, small) == want
    import torch  # (run alone, this file pays torch's one-time device start-up here, about 10 s)
    enc = icx.Encoder(ctx)  # the device entry's workspace: fresh, then grown, then a smaller image
    d_out = torch.empty(512 << 10, dtype=torch.uint8, device="cuda")
    for px in (small, big, small):
        h, w, c = px.shape
        d_src = torch.from_numpy(px).cuda()
        rc, n = enc.encode_device(100, 444, w, h, c, d_src.data_ptr(), d_out.data_ptr(), d_out.numel())
        assert rc == icx.OK and d_out[:n].cpu().numpy().tobytes() == oracle(444, 100, px)
    enc.close()


# ---- run geometry: the widths around one and two 512-pixel runs, the heights around one and two
# MCU rows; dc_swing puts the largest DC step on every unit boundary, edge_contrast makes the
# replicated last column / row matter
WIDTHS = {444: (504, 511, 512, 513, 520, 1024, 1025), 420: (496, 511, 512, 513, 527, 528, 529, 1025)}


@pytest.mark.parametrize("h", [8, 9, 16, 17, 33])
@pytest.mark.parametrize("sub", [444, 420])
def test_run_geometry(ctx, sub, h):
    for i, w in enumerate(WIDTHS[sub]):
        v = J.VARIANTS[(i + h) % 3]
        for period in (1, 3):
            px = J.dc_swing(w, h, sub, v, period=period)
            assert gpu(ctx, sub, 100, px) == oracle(sub, 100, px), ("dc_swing", v, w, h, period)
        px = J.edge_contrast(w, h)
        for q in (100, 50):
            assert gpu(ctx, sub, q, px) == oracle(sub, q, px), ("edge_contrast", w, h, q)
        if sub == 444:
            px = J.dc_swing(w, h, 444, v)
            assert gpu(ctx, "tje", 3, px) == oracle("tje", 3, px), ("tje dc_swing", v, w, h)


# ---- the pixel loader's paths through the device entry: RGB rows of dwords (comps 3, w % 4 == 0,
# source aligned), bytes otherwise (w % 4 != 0, comps 4, or a source off 4-byte alignment)
@pytest.mark.parametrize("sub", [444, 420])
def test_pixel_loader_paths(ctx, sub):
    import torch
    enc = icx.Encoder(ctx)
    d_out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    cases = [(J.edge_contrast(520, 17, 3), 0), (J.edge_contrast(513, 17, 3), 0), (J.edge_contrast(513, 17, 4), 0),
             (J.edge_contrast(520, 17, 4), 0), (J.sign_blocks("by", 2 if sub == 420 else 1), 0)]
    cases += [(J.edge_contrast(520, 17, 3), off) for off in (1, 2, 3)]
    cases += [(J.sign_blocks("rc", 2 if sub == 420 else 1), off) for off in (1, 2, 3)]
    for px, off in cases:
        h, w, c = px.shape
        buf = torch.zeros(px.size + 8, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0
        buf[off:off + px.size] = torch.from_numpy(px.reshape(-1)).cuda()
        for q in (100, 90):
            rc, n = enc.encode_device(q, sub, w, h, c, buf.data_ptr() + off, d_out.data_ptr(), d_out.numel())
            assert rc == icx.OK
            assert d_out[:n].cpu().numpy().tobytes() == oracle(sub, q, px), (w, h, c, off, q)
    enc.close()


# ---- batch entry: one geometry, very different streams (look-back chains and lengths)
def batch_images(sub):
    w, h = 1024, 64
    sb = J.sign_blocks("grey", 2 if sub == 420 else 1)
    sb = np.ascontiguousarray(np.tile(sb, (h // sb.shape[0], 1, 1)))
    imgs = [sb, J.noise01(21, w, h), J.flat(w, h), J.dc_swing(w, h, sub, "by"), J.dc_swing(w, h, sub, "rc", period=5)]
    assert all(x.shape == (h, w, 3) for x in imgs)
    return w, h, imgs


@pytest.mark.parametrize("sub", [444, 420])
def test_batch_of_crafted_images(ctx, sub, monkeypatch):
    import torch
    w, h, imgs = batch_images(sub)
    want = [oracle(sub, 100, px) for px in imgs]
    d_src = [torch.from_numpy(px).cuda() for px in imgs]
    stride = (max(len(x) for x in want) + 64) | 1  # odd: images 1.. start at every byte alignment
    d_out = torch.empty(5 * stride, dtype=torch.uint8, device="cuda")
    enc = icx.Encoder(ctx)
    for split in (None, "2"):
        if split:
            monkeypatch.setenv("ICX_ENC_BATCH", split)
        d_out.fill_(0xAB)
        st, sizes = enc.encode_device_batch(100, sub, w, h, 3, [t.data_ptr() for t in d_src], d_out.data_ptr(), stride)
        assert list(st) == [icx.OK] * 5 and list(sizes) == [len(x) for x in want]
        out = d_out.cpu().numpy()
        for k in range(5):
            assert out[k * stride: k * stride + sizes[k]].tobytes() == want[k], (split, k)
            assert bool((out[k * stride + sizes[k]: (k + 1) * stride] == 0xAB).all()), (split, k)
    enc.close()


@pytest.mark.parametrize("sub", [444, 420])
def test_batch_output_cap_is_exact(ctx, sub):
    """A stride of exactly the largest file: every image is written. One byte less: that image alone
    reports OUT_OF_MEM with its size, its slot stays untouched, the others are intact."""
    import torch
    w, h, imgs = batch_images(sub)
    want = [oracle(sub, 100, px) for px in imgs]
    lens = [len(x) for x in want]
    big = int(np.argmax(lens))
    assert sorted(lens)[-1] > sorted(lens)[-2]
    d_src = [torch.from_numpy(px).cuda() for px in imgs]
    d_out = torch.empty(5 * lens[big], dtype=torch.uint8, device="cuda")
    enc = icx.Encoder(ctx)
    for stride in (lens[big], lens[big] - 1):
        d_out.fill_(0xAB)
        st, sizes = enc.encode_device_batch(100, sub, w, h, 3, [t.data_ptr() for t in d_src], d_out.data_ptr(), stride)
        fits = stride == lens[big]
        assert list(st) == [icx.OK if (fits or k != big) else icx.OUT_OF_MEM for k in range(5)]
        assert list(sizes) == lens
        out = d_out.cpu().numpy()
        for k in range(5):
            slot = out[k * stride: (k + 1) * stride]
            if k == big and not fits:
                assert bool((slot == 0xAB).all())
            else:
                assert slot[:lens[k]].tobytes() == want[k], (stride, k)
                assert bool((slot[lens[k]:] == 0xAB).all()), (stride, k)
    enc.close()
