"""The wave inflate (icx_inflate_wave.h exr_inflate_wave) on crafted deflate streams: the corpus of
inflate_corpus.py, whose expected bytes come from the construction of each stream and which the
CPU tests (test_inflate_craft.py) hold against zlib and the portable inflate.

Through the PNG read: each stream is the IDAT of a one-row 8-bit grey image (deflate_craft.png_of),
one wave per stream, a whole group in one PngBatch call. The first output byte is the row's filter
type 0, so the pixels are the other bytes as they are. A stream is accepted only when it is valid
and gives exactly the row's bytes; every other one must end as PNGR_BAD_DATA with dims 0 and leave
its neighbours in the batch alone. On this path the gathered stream starts 16-byte aligned; the
OpenEXR read hands the inflate the chunk where it lies in the file, so the input window's
re-alignment (InW::mis) is tested through ZIP chunks at the four start residues.

The ring sizes the corpus aims at (inflate_corpus.WIN) are kPngdWin and the default ICX_EXR_WIN,
both 16384; ICX_EXR_WIN is a build-time knob of the OpenEXR read."""
import struct
import zlib

import numpy as np
import pytest

import deflate_craft as D
import imagecodecs_amd as icx
import inflate_corpus as K
import pngread_util as R
from oracle import exr_oracle as O
from tools import exrwrite as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def _png(c, split=0):
    if not c.z:  # (no byte at all: still an IDAT chunk, an empty one)
        return R.wrap(c.need - 1, 1, 8, 0, b"", pre=R.chunk(b"IDAT", b""))
    return D.png_of(c.z, c.need - 1, split)


def run_batch(ctx, cases, split=0):
    """One PngBatch call over the cases, a valid stream in front and behind; checks every status,
    dims and pixel, and that nothing is written past an image."""
    import torch
    good = K.group("window_lengths")[0]
    cases = [good] + list(cases) + [good]
    files = [_png(c, split) for c in cases]
    n, max_w = len(files), max(c.need for c in cases) - 1
    dev = torch.device("cuda", 0)
    sizes = np.array([len(f) for f in files], np.uint64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    stride = 4 * max_w + 4
    b = icx.PngBatch(ctx, n, max_w, 1)
    data = torch.from_numpy(np.frombuffer(b"".join(files), np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_sz = torch.from_numpy(sizes.view(np.int64)).to(dev)
    out = torch.full((n * stride,), 0xAB, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    dims = torch.full((n, 3), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    b.decode_device(n, data.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), out.data_ptr(), stride, st.data_ptr(),
                    dims.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    st, dims, out = st.cpu().numpy(), dims.cpu().numpy(), out.cpu().numpy().reshape(n, stride)
    b.close()
    bad = []
    for i, c in enumerate(cases):
        ok = c.full is not None and len(c.full) == c.need
        if not ok:
            if (st[i], list(dims[i])) != (icx.PNGR_BAD_DATA, [0, 0, 0]):
                bad.append((c.name, "not refused", int(st[i])))
            continue
        w = c.need - 1
        want = np.repeat(np.frombuffer(c.full, np.uint8)[1:, None], 4, axis=1)
        want[:, 3] = 255
        if (st[i], list(dims[i])) != (icx.PNGR_OK, [w, 1, 4]):
            bad.append((c.name, "refused", int(st[i])))
        elif not np.array_equal(out[i, : 4 * w].reshape(w, 4), want):
            bad.append((c.name, "pixels differ from byte", int(np.argmax(out[i, : 4 * w: 4] != want[:, 0])) + 1))
        elif not (out[i, 4 * w:] == 0xAB).all():
            bad.append((c.name, "bytes written past the image"))
    assert not bad, bad[:8]


GROUPS = ["long_codes", "header_forms", "leniencies", "zlib_headers", "invalid_symbols", "ring_or_output", "repeats",
          "flush_and_cap", "stored_blocks", "stored_65535", "adler_cases"]


@pytest.mark.parametrize("name", GROUPS)
def test_crafted_group(ctx, name):
    """(leniencies: accepted with the bytes test_inflate_craft.py records, where zlib refuses)"""
    run_batch(ctx, K.group(name))


def test_long_codes_split_idat(ctx):
    run_batch(ctx, K.group("long_codes") + K.group("header_forms"), split=1)


def test_input_end(ctx):
    """Every truncation of a fixed and of a dynamic stream is refused (a run of zero bits past the
    end decodes as fixed-code end of block, so every length counts); 0 to 3 junk bytes after the
    trailer change nothing: the contract is zlib.decompress on the concatenated IDAT."""
    for c in K.group("trailing_junk"):
        assert zlib.decompress(c.z) == c.full
    run_batch(ctx, K.group("truncations") + K.group("trailing_junk"))


@pytest.mark.parametrize("split", [0, 5])
def test_window_reader_png(ctx, split):
    """Streams of 250..262 and 506..518 bytes: the ends of InW's two 256-byte registers (ld's byte
    tail at e, adv once per iteration), mis == 0."""
    run_batch(ctx, K.group("window_lengths"), split=split)


# ------------------------------------------------------------------ OpenEXR: the four start residues
def _exr_with_stream(n, pad):
    """A 2-line half RGBA ZIP file (one chunk) whose chunk payload is a crafted stream of n bytes
    that inflates to the predictor bytes the writer made; `pad` bytes of a header attribute move
    the payload's offset in the file. The chunk is 16 pixels wide (256 raw bytes), 18 where n is
    256: a chunk as long as its raw size is read as uncompressed."""
    w = 18 if n == 256 else 16
    rng = np.random.default_rng(n)
    chans = [(name, (rng.integers(0, 3, (2, w)) * 0.25 + k).astype(np.float16)) for k, name in enumerate("RGBA")]
    seen = {}
    W.write_exr(chans, W.ZIP, raw_chunks=lambda k, d: seen.setdefault(k, d))
    pred = zlib.decompress(seen[0])  # (the writer's own zlib stream: what the chunk must inflate to)
    assert len(seen) == 1 and len(pred) == 16 * w != n
    z = D.stretch(D.tokenize(pred), n)
    data = W.write_exr(chans, W.ZIP, raw_chunks=lambda k, d: z, extra_attrs=W.attr("pad", "string", b"p" * pad))
    at = data.index(z)
    assert struct.unpack("<i", data[at - 4:at])[0] == n
    return data, at


@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513])
def test_window_reader_exr_start_residues(ctx, n):
    """mis = 0..3: the chunk's first byte at each residue mod 4 of the file (the device copy of the
    file is at least 4-byte aligned), stream ends at and next to the window's register edges."""
    residues = set()
    for pad in range(4):
        data, at = _exr_with_stream(n, pad)
        residues.add(at % 4)
        oc, ow, oh, oimg = O.decode(data)
        code, w, h, img = ctx.exr_decode(data)
        assert (code, w, h) == (oc, ow, oh) == (0, ow, 2), (n, pad, code)
        assert np.array_equal(img.view(np.uint32), oimg.view(np.uint32)), (n, pad)
    assert residues == {0, 1, 2, 3}
