"""GPU parity of the guess-write lanes' second lookup on a partly filled window (k_gw_lane without
the error-byte bounds: write_step_short also serves a window of nb <= 32 bits when the first-level
entry is a plain one whose symbols take no more than nb bits). The crafted streams of
tests/gw3_craft.py -- long first symbols that leave the window short, then a symbol or a pair that
does not fit it, or a code longer than the AC window; tests/test_gw3_emu.py checks on the CPU that
every refusal is reached -- those of tests/gw2_craft.py, and two synthetic 256 x 256 images per
sampling, forced onto the guess-write path (ICX_GW=1) in 512-byte lanes, so every image spans
several lanes and many windows run short. ICX_SUB_BYTES=512 asks for that lane size; the library
reads it once per process, so in a run of the whole suite it is already fixed at its default, under
which the planner gives scans of up to 256 KiB (every one here) the same 512-byte lanes. One
restart-interval stream runs on the interval-aligned lanes (ICX_DRI_GW=1), the same kernel. Status
and pixels equal the oracle's, bit for bit, and every image stays on the parallel path."""
import pytest

import imagecodecs_amd as icx
from oracle import pyoracle as O
from tools import synthpy as S
import gw2_craft
import gw3_craft

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def _with_oracle(streams):
    return {n: (d, O.decode(d)) for n, d in sorted(streams.items())}  # the oracle's result, once


@pytest.fixture(scope="module")
def inputs():
    out = dict(gw3_craft.streams())
    out.update(gw2_craft.streams())
    for sampling in ("420", "444", "gray"):
        for seed in (6200, 6201):
            out[f"synth_{sampling}_256_{seed}"] = S.synth_jpeg(seed, 256, 256, sampling, 90)
    return _with_oracle(out)


def _same_as_oracle(names, res, inputs):
    for n, (code, w, h, c, pix) in zip(names, res):
        ocode, ow, oh, on, opix = inputs[n][1]
        assert code == ocode, (n, code, ocode)
        if ocode == 0:
            assert (w, h, c) == (ow, oh, on), n
            assert pix.tobytes() == opix, n


def test_short_window_lanes_match_oracle(ctx, monkeypatch, inputs):
    monkeypatch.setenv("ICX_GW", "1")
    monkeypatch.setenv("ICX_SUB_BYTES", "512")
    names = list(inputs)
    assert all(len(inputs[n][0]) < 256 * 1024 for n in names)  # 512-byte lanes either way
    # (the comparison is not vacuous: the short-window streams and the synthetic images decode)
    assert all(inputs[n][1][0] == 0 for n in names if n.startswith(("short_", "synth_")))
    b = icx.Batch(ctx, len(names), 256, 256)
    res = b.decode_host([inputs[n][0] for n in names])
    stats = b.path_stats()
    b.close()
    print(stats)
    # no silent fallback: every image decided by the lanes (NanoJPEG's syntax errors included)
    assert stats == {"parallel": len(names), "fallback": 0, "sequential": 0}, stats
    _same_as_oracle(names, res, inputs)


def test_short_window_dri_lanes_match_oracle(ctx, monkeypatch):
    monkeypatch.setenv("ICX_GW", "1")
    monkeypatch.setenv("ICX_SUB_BYTES", "512")
    monkeypatch.setenv("ICX_DRI_GW", "1")
    inputs = _with_oracle(gw3_craft.dri_streams())
    names = list(inputs)
    assert all(inputs[n][1][0] == 0 for n in names)
    b = icx.Batch(ctx, len(names), 256, 256)
    res = b.decode_host([inputs[n][0] for n in names])
    stats, dri = b.path_stats(), b.dri_stats()
    b.close()
    print(stats, dri)
    assert stats == {"parallel": len(names), "fallback": 0, "sequential": 0}, stats
    assert dri == {"gw": len(names), "gw_fallback": 0}, dri  # decided by the guess-write lanes, not sent back
    _same_as_oracle(names, res, inputs)
