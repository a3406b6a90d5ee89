"""GPU parity on the crafted decoder inputs of tests/jpegdec_craft.py: magnitude categories 11 .. 15
behind codes of up to 16 bits, pairs at the 4-bit total's limit, DC sizes up to 15 and DC symbols
with a high nibble, absolute DCs around the int16 cell's escape value, scans that are 99 % stuffed
bytes, size-0 AC symbols in either lookup position; and for the back half block_transform's 2^14
gate from both sides, the fast path's worst-case intermediates, idct_fast_ok's 2^22 gate per slot,
32-bit wrap-around, uniform int16 blocks, every DC-only pixel value across both clip ends and the
colour conversion's corners. tests/test_decode_craft.py proves on the CPU that the files hold
these states. Status, size and every pixel byte equal the oracle's: the reference is integer
code, so equality is exact."""
import pytest

import imagecodecs_amd as icx
from oracle import pyoracle as O
import jpegdec_craft as J

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def inputs():
    return {n: (d, O.decode(d)) for n, d in sorted(J.streams().items())}  # the oracle's result, once


def _compare(names, inputs, res):
    bad = []
    for n, (code, w, h, c, pix) in zip(names, res):
        ocode, ow, oh, on, opix = inputs[n][1]
        if code != ocode:
            bad.append((n, "status", code, ocode))
        elif ocode == 0 and (w, h, c) != (ow, oh, on):
            bad.append((n, "size", (w, h, c), (ow, oh, on)))
        elif ocode == 0 and pix.tobytes() != opix:
            got = pix.tobytes()
            first = next(i for i in range(len(opix)) if got[i] != opix[i])
            bad.append((n, "pixels", sum(a != b for a, b in zip(got, opix)), "first at", first))
    assert not bad, bad


def _batch(ctx, names, inputs):
    b = icx.Batch(ctx, len(names), 536, 256)
    res = b.decode_host([inputs[n][0] for n in names])
    stats = b.path_stats()
    b.close()
    return res, stats


@pytest.mark.parametrize("mode", ["0", "4", "5"])
@pytest.mark.parametrize("gw", ["1", "0"])
def test_all_streams_each_entropy_path_and_plane_mode(ctx, monkeypatch, inputs, gw, mode):
    """One batch of every stream, the guess-write lanes (ICX_GW=1: 512-byte lanes at these sizes)
    and the three passes (0), crossed with the 4:2:0 plane modes: k_idct (0), k_idct420s for all
    three planes (4), k_fused420s for luma with k_idct420s for chroma (5)."""
    monkeypatch.setenv("ICX_GW", gw)
    monkeypatch.setenv("ICX_FUSE420", mode)
    names = list(inputs)
    res, stats = _batch(ctx, names, inputs)
    print(gw, mode, stats)
    _compare(names, inputs, res)
    if gw == "1":  # no silent fallback: the lanes decide every image, NanoJPEG's syntax errors included
        assert stats == {"parallel": len(names), "fallback": 0, "sequential": 0}, stats


@pytest.mark.parametrize("family", J.FAMILIES)
def test_guess_write_lanes_decide_each_family(ctx, monkeypatch, inputs, family):
    """path_stats() family by family under ICX_GW=1 (ff_dense unstuffs to about 2 bytes a pixel,
    the U pool's default share of one slot: it must still take the parallel path)."""
    monkeypatch.setenv("ICX_GW", "1")
    names = [n for n in inputs if J.family(n) == family]
    res, stats = _batch(ctx, names, inputs)
    print(family, stats)
    _compare(names, inputs, res)
    assert stats == {"parallel": len(names), "fallback": 0, "sequential": 0}, stats


def test_idct_families_other_samplings(ctx):
    """The IDCT families at 4:4:4, 4:2:2 and gray: k_idct's other unit shapes. Default modes."""
    every = {}
    for sampling in ("444", "422", "gray"):
        every.update(J.idct_streams(sampling))
    ins = {n: (d, O.decode(d)) for n, d in sorted(every.items())}
    names = list(ins)
    res, stats = _batch(ctx, names, ins)
    _compare(names, ins, res)
    assert stats["fallback"] == 0 and stats["sequential"] == 0, stats


def test_every_stream_alone(ctx, inputs):
    """Each stream through the one-image entry: a one-slot workspace sized for that image."""
    names = list(inputs)
    res = []
    for n in names:
        code, w, h, c, pix = ctx.decode(inputs[n][0])
        res.append((code, w, h, c, memoryview(pix) if pix is not None else None))
    _compare(names, inputs, res)


def test_inputs_are_what_they_claim(inputs):
    """The error cases fail in the oracle, the others decode: the comparisons are not vacuous."""
    for n, (_, (ocode, *_rest)) in inputs.items():
        assert (ocode != 0) == n.startswith(J.ERRORS), (n, ocode)
