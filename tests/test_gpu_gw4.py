"""GPU parity of the guess-write lanes' third lookup of an iteration (k_gw_lane without the
error-byte bounds: after the second lookup one more AC lookup of the same block under
write_step_short's rule, without a refill). The crafted streams of tests/gw4_craft.py -- at the third
position each refusal, a block end, a committed pair, a window drained to its last bit and an
invalid code that waits for the next full window; tests/test_gw4_emu.py checks on the CPU that each
is reached -- those of tests/gw3_craft.py and tests/gw2_craft.py, and two synthetic 256 x 256 images
per sampling, forced onto the guess-write path (ICX_GW=1) in 512-byte lanes, so every image spans
several lanes. ICX_SUB_BYTES=512 asks for that lane size; the library reads it once per process, so
in a run of the whole suite it is already fixed at its default, under which the planner gives scans
of up to 256 KiB (every one here) the same 512-byte lanes. The restart-interval stream runs on the
interval-aligned lanes (ICX_DRI_GW=1), the same kernel. The same inputs then run with ICX_GW=0 and
ICX_DRI_GW=0, the three-pass path and one lane per interval, so that both instances of k_spec_write
decode them too, streams that end in a syntax error included. Status and pixels equal the oracle's,
bit for bit, and every image stays on the parallel path."""
import pytest

import imagecodecs_amd as icx
from oracle import pyoracle as O
from tools import synthpy as S
import gw2_craft
import gw3_craft
import gw4_craft

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
    out = dict(gw4_craft.streams())
    out.update(gw3_craft.streams())
    out.update(gw2_craft.streams())
    for sampling in ("420", "444", "gray"):
        for seed in (6300, 6301):
            out[f"synth_{sampling}_256_{seed}"] = S.synth_jpeg(seed, 256, 256, sampling, 90)
    return _with_oracle(out)


def _cut(data, drop):
    """`data` without its EOI and its last `drop` entropy-coded bytes, ending in a lone FF: NanoJPEG's
    syntax error at that byte, inside the last restart interval."""
    assert data.endswith(b"\xff\xd9")
    body = data[:-2 - drop]
    while body.endswith(b"\xff"):
        body = body[:-1]
    return body + b"\xff"


@pytest.fixture(scope="module")
def dri_inputs():
    out = dict(gw4_craft.dri_streams())
    (name, data), = out.items()
    out[name + "_cut"] = _cut(data, 700)
    return _with_oracle(out)


def _same_as_oracle(names, res, inputs):
    for n, (code, w, h, c, pix) in zip(names, res):
        ocode, ow, oh, on, opix = inputs[n][1]
        assert code == ocode, (n, code, ocode)
        if ocode == 0:
            assert (w, h, c) == (ow, oh, on), n
            assert pix.tobytes() == opix, n


def _decode(ctx, inputs, names):
    b = icx.Batch(ctx, len(names), 256, 256)
    res = b.decode_host([inputs[n][0] for n in names])
    stats, dri = b.path_stats(), b.dri_stats()
    b.close()
    print(stats, dri)
    # no silent fallback: every image decided by the lanes (NanoJPEG's syntax errors included)
    assert stats == {"parallel": len(names), "fallback": 0, "sequential": 0}, stats
    _same_as_oracle(names, res, inputs)
    return dri


def test_inputs_are_what_they_claim(inputs, dri_inputs):
    """The error cases fail in the oracle, the others decode: the comparisons below are not vacuous."""
    for n, (d, (ocode, *_rest)) in inputs.items():
        assert len(d) < 256 * 1024, n  # 512-byte lanes with or without ICX_SUB_BYTES
        if n.startswith(("third_", "short_", "synth_")):
            assert (ocode != 0) == n.startswith(gw4_craft.ERRORS), (n, ocode)
    for n, (d, (ocode, *_rest)) in dri_inputs.items():
        assert (ocode != 0) == n.endswith("_cut"), (n, ocode)


@pytest.mark.parametrize("gw_env", ["1", "0"])
def test_third_lookup_lanes_match_oracle(ctx, monkeypatch, inputs, gw_env):
    """ICX_GW=1: k_gw_lane, both instances; ICX_GW=0: k_spec_guess / count / write<512>."""
    monkeypatch.setenv("ICX_GW", gw_env)
    monkeypatch.setenv("ICX_SUB_BYTES", "512")
    _decode(ctx, inputs, list(inputs))


def test_third_lookup_dri_lanes_match_oracle(ctx, monkeypatch, dri_inputs):
    monkeypatch.setenv("ICX_GW", "1")
    monkeypatch.setenv("ICX_SUB_BYTES", "512")
    monkeypatch.setenv("ICX_DRI_GW", "1")
    names = [n for n in dri_inputs if not n.endswith("_cut")]
    dri = _decode(ctx, dri_inputs, names)
    assert dri == {"gw": len(names), "gw_fallback": 0}, dri  # decided by the guess-write lanes, not sent back


def test_dri_interval_lanes_match_oracle(ctx, monkeypatch, dri_inputs):
    """ICX_DRI_GW=0: one lane per restart interval (k_spec_write<256>), the truncated stream included."""
    monkeypatch.setenv("ICX_GW", "1")
    monkeypatch.setenv("ICX_SUB_BYTES", "512")
    monkeypatch.setenv("ICX_DRI_GW", "0")
    dri = _decode(ctx, dri_inputs, list(dri_inputs))
    assert dri == {"gw": 0, "gw_fallback": 0}, dri
