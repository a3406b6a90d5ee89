"""GPU: the OpenEXR write (icx_exrw.hip) through the C ABI, chunk by chunk against tinyexr's files
(tests/golden/exrw) and the restatement in tests/exrw_util.py: container bytes exact, every payload
raw (size == S) or a shorter zlib stream that inflates to tinyexr's predictor bytes, and every file
reads back -- through the oracle and through the GPU reader -- to the input's bits."""
import numpy as np
import pytest

import imagecodecs_amd as icx
from oracle import exr_oracle as O
import deflate_read as R
import exrw_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def check(ctx, a, fp16, golden=None):
    """Encode, run the parity contract and both read-backs -> (file, raw chunks)."""
    data = ctx.exr_encode(a, fp16=fp16)
    nraw = U.check_file(a, fp16, data, golden)
    want = U.expected_readback(a, fp16)
    code, w, h, img = O.decode(data)
    assert code == 0 and (np.ascontiguousarray(img).view(np.uint32) == want).all(), "oracle read-back"
    code, w, h, img = ctx.exr_decode(data)
    assert code == 0 and (np.ascontiguousarray(img).view(np.uint32) == want).all(), "GPU read-back"
    assert len(data) <= icx.lib().icx_exr_encode_bound(a.shape[1], a.shape[0], a.shape[2], int(fp16))
    return data, nraw


def audit_file(a, fp16, data):
    """The token-level audit (deflate_read.audit) of every compressed chunk of a file of ours: its
    tokens give the predictor bytes, its codes are complete, free of unused symbols and cost the
    optimum, its headers are tight; and no match crosses a 4 KiB segment end (matches
    are cut there). -> [(blocks, audit's figures)] per compressed chunk."""
    out = []
    for k, (y, size, payload, at) in enumerate(U.split(a, fp16, data)[2]):
        raw = U.chunk_raw(a, fp16, k)
        if size == len(raw):
            continue
        blocks = R.read_zlib(payload)
        stats = R.audit(blocks, U.predict(raw), log=print)
        assert R.crossing(blocks, 4096) == [], ("a match crosses a segment end", k)
        out.append((blocks, stats))
    return out


def from_predictor_bytes(v, w):
    """The 16 x w one-channel float image whose single chunk has the predictor bytes `v` (64 w of
    them): the predictor and the reorder of CompressZip undone."""
    v = np.asarray(v, np.int64)
    assert len(v) == 64 * w
    t = np.cumsum(np.concatenate([v[:1], v[1:] - 128])) & 255
    raw = np.empty(len(v), np.uint8)
    raw[0::2], raw[1::2] = t[: len(v) // 2], t[len(v) // 2:]
    a = raw.view(np.float32).reshape(16, w, 1)
    assert U.predict(U.chunk_raw(a, False, 0)) == v.astype(np.uint8).tobytes()
    return a


@pytest.mark.parametrize("name", ["none_9x8_rgba", "none_15x15_rgb", "none_1x1_a"])
def test_none_files_equal_tinyexr(ctx, name):
    a, fp16, gold = U.load_golden(name)
    data, nraw = check(ctx, a, fp16, gold)
    assert data == gold


@pytest.mark.parametrize("name", ["zip_16x1_rgba", "zip_1x16_rgba", "zip_33x20_rgba", "zip_33x17_rgb_half",
                                  "zip_16x17_a"])
def test_zip_edges(ctx, name):
    a, fp16, gold = U.load_golden(name)
    check(ctx, a, fp16, gold)


def test_all_raw_file_equals_tinyexr(ctx):
    a, fp16, gold = U.load_golden("raw_33x40_rgba")
    data, nraw = check(ctx, a, fp16, gold)
    assert nraw == 3 and data == gold


def test_fp16_edge_table(ctx):
    a, fp16, gold = U.load_golden("half_edges_64x16_rgba")
    check(ctx, a, fp16, gold)  # (incl. the inflated chunk == the golden's inflated chunk)


@pytest.mark.parametrize("w,h", [(300, 100), (1100, 33)])
def test_several_segments_long_distances(ctx, w, h):
    """76,800- and 281,600-byte chunks: many segments per chunk, one past 256 KiB; the previous
    line is 2400 / 8800 bytes back, inside the window."""
    a = U.smooth(w, h, 4, 20 + w)
    data, nraw = check(ctx, a, False)
    assert nraw == 0
    audited = audit_file(a, False, data)
    assert len(audited) == U.nchunks(a, False) and any(len(b) > 1 for b, _ in audited)  # (several deflate blocks)


def test_wide_drops_the_line_candidate(ctx):
    """4200 x 16 RGBA float: the previous line is 33,600 bytes back, past the 32 KiB window."""
    a = U.smooth(4200, 16, 4, 30)
    data, nraw = check(ctx, a, False)
    assert len(audit_file(a, False, data)) + nraw == U.nchunks(a, False)


@pytest.mark.parametrize("fp16", [False, True])
def test_flat_finds_runs(ctx, fp16):
    """Every sample 0.25: the payloads together are under 2% of the raw bytes (zlib: 261 / 199
    bytes of 160,000 / 80,000)."""
    a = np.full((50, 200, 4), 0.25, np.float32)
    data, nraw = check(ctx, a, fp16)
    sizes = [c[1] for c in U.split(a, fp16, data)[2]]
    raw = a.size * (2 if fp16 else 4)
    print("flat", "fp16" if fp16 else "float", "payload bytes", sum(sizes), "of", raw)
    assert sum(sizes) < 0.02 * raw
    audited = audit_file(a, fp16, data)
    assert len(audited) == U.nchunks(a, fp16)


def flat_and_geometric_tail(n, nflat, ratio, top, seed, first=60):
    """n predictor bytes, shuffled: a tail of values with counts 1, ratio, ratio^2 ... up to `top`
    (rounded, increasing) and `nflat` values sharing the rest equally. With the end-of-block code
    as one more leaf of weight 1 the tail is a chain in the Huffman tree, one level per value, and
    the flat values add log2(nflat) levels above it; a ratio near 2 keeps the chain when a few
    length symbols of chance matches fall among its weights (Fibonacci counts lose it). Many flat
    values keep 4-byte repeats inside a segment rare, so the stream stays literals."""
    tail, x = [], 1.0
    while round(x) <= top:
        if not tail or round(x) > tail[-1]:
            tail.append(int(round(x)))
        x *= ratio
    cnt = np.array([(n - sum(tail)) // nflat] * nflat + tail[::-1], np.int64)
    cnt[0] += n - cnt.sum()
    v = np.repeat(first + np.arange(len(cnt)), cnt)
    np.random.default_rng(seed).shuffle(v)
    return v


@pytest.mark.parametrize("ratio", [1.9, 1.8])
def test_limiter_on_skewed_predictor_bytes(ctx, ratio):
    """A 2048 x 16 one-channel chunk: 131,072 predictor bytes in two deflate blocks of 16 segments
    (64 KiB, the largest this writer makes), each block 64 flat values and a tail of counts
    1, 2, 4, 7, 13 ... up to 1000 (ratio 1.9 or 1.8). The unlimited literal/length tree of the
    GPU's own tokens is deeper than 15 in both blocks (measured 17 and 18), so the 15-bit limiter
    of icx_exrw.hip runs; the audit holds its code complete, within the limit and close to the
    package-merge optimum (measured: equal to it at 1.9, 1.0000351 of it at 1.8)."""
    v = np.concatenate([flat_and_geometric_tail(65536, 64, ratio, 1000, 50 + k) for k in range(2)])
    a = from_predictor_bytes(v, 2048)
    data, nraw = check(ctx, a, False)
    assert nraw == 0
    (blocks, stats), = audit_file(a, False, data)
    assert [b.out for b in blocks] == [(0, 65536), (65536, 131072)]
    for bi, b in enumerate(blocks):
        depth = {s["code"]: s["depth"] for s in stats if s["block"] == bi}
        ratio = max(s["ratio"] for s in stats if s["block"] == bi)
        print("exr limiter: block", bi, "unlimited depths", depth, "tokens", len(b.tokens), "matches", len(b.matches()),
              "worst ratio", ratio)
        assert len(b.tokens) + 1 >= 1597
        assert depth["ll"] > 15 and max(b.ll_lens) == 15, depth


def test_block_without_a_match(ctx):
    """32,768 predictor bytes of 160-value noise (two deflate blocks): the Huffman codes alone make
    the stream smaller than the samples, and a block with no match carries the two forced 1-bit
    distance codes."""
    v = np.random.default_rng(51).integers(40, 200, 64 * 512)
    a = from_predictor_bytes(v, 512)
    data, nraw = check(ctx, a, False)
    assert nraw == 0
    (blocks, stats), = audit_file(a, False, data)
    assert len(blocks) == 2
    bare = [b for b in blocks if not b.matches()]
    assert bare and all(b.hdist + 1 == 2 and b.d_lens == [1, 1] for b in bare)


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).to(torch.device("cuda", 0))


def test_device_batch_matches_single(ctx):
    """Three images of different sizes in one call, output slots at odd byte offsets: each result
    equals the single-image call's bytes (ZIP, NONE and a partial last chunk among them)."""
    import torch
    imgs = [U.smooth(70, 37, 4, 40), U.smooth(9, 8, 4, 41), U.smooth(300, 20, 4, 42)]
    singles = [ctx.exr_encode(a) for a in imgs]
    srcs = [_dev(a) for a in imgs]
    caps = [icx.lib().icx_exr_encode_bound(a.shape[1], a.shape[0], 4, 0) for a in imgs]
    slots, at = [], 1
    for c in caps:
        slots.append(at)
        at += c + c % 2  # keep every slot odd
    assert all(s % 2 == 1 for s in slots)
    out = torch.full((at + 64,), 0xA5, dtype=torch.uint8, device=srcs[0].device)
    codes, sizes = ctx.exr_encode_device_batch([s.data_ptr() for s in srcs], [a.shape[1] for a in imgs],
                                               [a.shape[0] for a in imgs], 4, False,
                                               [out.data_ptr() + s for s in slots], caps)
    assert list(codes) == [0, 0, 0]
    host = out.cpu().numpy()
    for a, one, s, n, c in zip(imgs, singles, slots, sizes, caps):
        assert int(n) == len(one) and host[s:s + int(n)].tobytes() == one
        assert (host[s + int(n):s + c] == 0xA5).all()  # nothing past the file in its slot
    assert host[0] == 0xA5 and (host[at:] == 0xA5).all()
    # the device entry for one image gives the same bytes
    code, n = ctx.exr_encode_device(srcs[0].data_ptr(), 70, 37, 4, False, out.data_ptr() + 3, caps[0])
    assert code == 0 and out.cpu().numpy()[3:3 + n].tobytes() == singles[0]


def test_cap_one_byte_short(ctx):
    """cap = the file's size - 1: ICX_EXR_INTERNAL_ERR, nothing written (the canary after the
    buffer and the buffer itself are untouched), and the context stays usable."""
    import torch
    a = U.smooth(70, 37, 4, 40)
    one = ctx.exr_encode(a)
    src = _dev(a)
    out = torch.full((len(one) + 256,), 0x5A, dtype=torch.uint8, device=src.device)
    code, n = ctx.exr_encode_device(src.data_ptr(), 70, 37, 4, False, out.data_ptr(), len(one) - 1)
    assert code == icx.EXR_INTERNAL_ERR and n == len(one)
    assert "too small" in icx._err(ctx._p)
    assert (out.cpu().numpy() == 0x5A).all()
    code, n = ctx.exr_encode_device(src.data_ptr(), 70, 37, 4, False, out.data_ptr(), len(one))
    assert code == 0 and n == len(one)
    host = out.cpu().numpy()
    assert host[:n].tobytes() == one and (host[n:] == 0x5A).all()


def test_bad_arguments(ctx):
    import ctypes as C
    L = icx.lib()
    a = np.zeros((4, 4, 2), np.float32)
    out, size = C.c_void_p(), C.c_size_t()
    assert L.icx_exr_save_to_memory(ctx._p, a.ctypes.data, 4, 4, 2, 0, C.byref(out), C.byref(size)) == icx.EXR_INVALID_ARGUMENT
    assert L.icx_exr_save_to_memory(ctx._p, a.ctypes.data, 0, 4, 4, 0, C.byref(out), C.byref(size)) == icx.EXR_INVALID_ARGUMENT
    assert L.icx_exr_save_to_memory(ctx._p, None, 4, 4, 4, 0, C.byref(out), C.byref(size)) == icx.EXR_INVALID_ARGUMENT
    assert out.value is None and size.value == 0
    assert L.icx_exr_encode_bound(4, 4, 2, 0) == 0 and L.icx_exr_encode_bound(0, 4, 4, 0) == 0
    src = _dev(np.zeros((4, 4, 4), np.float32))
    dst = _dev(np.zeros(4096, np.uint8))
    assert ctx.exr_encode_device(src.data_ptr(), 4, 4, 2, False, dst.data_ptr(), 4096)[0] == icx.EXR_INVALID_ARGUMENT
    assert ctx.exr_encode_device(src.data_ptr(), 0, 4, 4, False, dst.data_ptr(), 4096)[0] == icx.EXR_INVALID_ARGUMENT
    assert len(ctx.exr_encode(np.zeros((4, 4, 4), np.float32))) > 0  # the context still works


def test_image_write_exr(tmp_path):
    """The Python Image mirrors the drop-in: read .exr, write .exr, read it back."""
    import os
    from conftest import GOLDEN
    im = icx.Image()
    im.read(os.path.join(GOLDEN, "exr", "scan_zip_half.exr"))
    out = str(tmp_path / "out.exr")
    im.write(out)
    back = icx.Image()
    back.read(out)
    assert (back.w_, back.h_, back.d_, back.type_) == (im.w_, im.h_, 4, icx.Image.FLOAT)
    assert back.pixels_.tobytes() == im.pixels_.tobytes()
