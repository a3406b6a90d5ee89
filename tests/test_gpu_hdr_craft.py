"""The GPU Radiance .hdr read against the crafted corpus (tests/hdr_craft.py): every file, placed at
its byte offset in the batch blob, must give the oracle's status, size, row count and float bits,
and must have been located the way the restated rule says -- `locate_stats()` equal to `predict`,
mode and candidate count. The serial walk decodes the same pixels as the parallel paths, so the
pixel assertions alone could not tell a linked file from one that fell back."""
import numpy as np
import pytest

import hdr_craft as K
import hdrutil as H
import imagecodecs_amd as icx
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
CASES = K.cases()


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def _decode(ctx, group, pad=0):
    """One batch of the cases at their blob offsets -> ([(status, w, h, rows, floats)], locate_stats)."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(group)
    blob, offs, sizes = K.place(group)
    max_w, max_h = max(c.dims[0] for c in group), max(c.dims[1] for c in group)
    data = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev)
    assert data.data_ptr() % 256 == 0  # blob offsets are device address residues
    d_off = torch.from_numpy(np.array(offs, np.int64)).to(dev)
    d_sz = torch.from_numpy(np.array(sizes, np.int64)).to(dev)
    stride = 4 * max_w * max_h + pad
    out = torch.full((n * stride,), -7.0, dtype=torch.float32, device=dev)
    st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    dims = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    b = icx.HdrBatch(ctx, n, max_w, max_h)
    torch.cuda.synchronize(dev)  # the fills above are done before the decode's stream starts
    b.decode_device(n, data.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), out.data_ptr(), stride,
                    st.data_ptr(), dims.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    stats = b.locate_stats()  # no synchronize first: it orders itself after the decode
    torch.cuda.synchronize(dev)
    b.close()
    out, st, dims = out.cpu().numpy(), st.cpu().numpy(), dims.cpu().numpy()
    res = []
    for i in range(n):
        w, h, rows = (int(v) for v in dims[i])
        res.append((int(st[i]), w, h, rows, out[i * stride: i * stride + w * h * 4].reshape(h, w, 4) if w * h else None))
    return res, stats


def _check(case, got, stat=None):
    ref, want = K.expectations()[case.name]
    assert got[0] == ref[0], case.name
    assert got[1:4] == ref[1:4], case.name
    np.testing.assert_array_equal(got[4].view(np.uint32), ref[4].view(np.uint32), err_msg=case.name)
    if case.pixels is not None:
        np.testing.assert_array_equal(got[4].view(np.uint32), H.expected_floats(case.pixels).view(np.uint32))
    if stat is not None:
        assert stat == want, (case.name, case.edge)
        assert stat[0] == case.mode, (case.name, case.edge)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_alone(ctx, case):
    res, stats = _decode(ctx, [case])
    _check(case, res[0], stats[0])


@pytest.mark.parametrize("group", K.GROUPS)
def test_group_in_one_batch(ctx, group):
    """Differing blob offsets in one blob, and slots that start off 16-byte alignment."""
    cs = [c for c in CASES if c.group == group]
    res, stats = _decode(ctx, cs, pad=1 + len(group) % 3)
    assert len(stats) == len(cs)
    for c, got, stat in zip(cs, res, stats):
        _check(c, got, stat)


@pytest.mark.parametrize("group", K.GROUPS)
def test_group_one_shot(ctx, group):
    for c in CASES:
        if c.group == group and (c.blob_offset == 0 or group != "scan"):  # (the same file at four offsets)
            _check(c, ctx.hdr_decode(c.file))


def test_locate_stats_before_and_after(ctx):
    """Nothing decoded: no images. A second, smaller decode replaces the first one's record."""
    b = icx.HdrBatch(ctx, 4, 16, 16)
    assert b.locate_stats() == []
    b.close()
    by = {c.name: c for c in CASES}
    two = [by["plain_111_straddle"], by["new_with_marker"]]
    _, stats = _decode(ctx, two)
    assert stats == [K.expectations()[c.name][1] for c in two]
    bad = K.Case("bad", "plain", b"#?RGBE\n\n-Y 2 +X 2\n" + bytes(16), 0, O.HDR_NOT_RADIANCE, None, 0, "a header error")
    import torch
    dev = torch.device("cuda", 0)
    blob, offs, sizes = K.place([bad, two[1]])
    data = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev)
    d_off, d_sz = (torch.from_numpy(np.array(v, np.int64)).to(dev) for v in (offs, sizes))
    out = torch.zeros(2 * 4 * 16 * 16, dtype=torch.float32, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    dims = torch.zeros((2, 3), dtype=torch.int32, device=dev)
    b = icx.HdrBatch(ctx, 4, 16, 16)
    torch.cuda.synchronize(dev)
    b.decode_device(2, data.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), out.data_ptr(), 4 * 16 * 16, st.data_ptr(),
                    dims.data_ptr(), 0)  # the context's own non-blocking stream
    assert b.locate_stats() == [(0, 0), K.predict(two[1].file)]
    b.close()
